// nexr_flat_api.cpp — the one-launch collectives of the C ABI (include/nexr.h): nexrSym*, nexrSymLL*, nexrFlat*,
// nexrFlatGroup* and nexrFlatHost*. Host code only: argument checks, launch geometry and the staged tables; the
// kernels live in nexr_sym.hip and nexr_flat*.hip. What it shares with nexr_api.cpp is declared in nexr_host.h.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <utility>
#include <vector>

#include "nexr_host.h"
#include "nexr_exchange_v_checks.h"

using namespace nexr;

// ---- what every entry below shares ------------------------------------------------------------------------------
namespace {
bool flatRanksOk(int n) { return n >= 2 && n <= NEXR_SYM_MAX_RANKS; }
bool eszOk(size_t esz) { return esz == 1 || esz == 2 || esz == 4 || esz == 8; }

// Both arrays and each of their n entries non-null and clear of alignMask, stored into p->in[] and p->out[].
template <typename Params>
bool takeBuffers(int n, const void* const* inputs, void* const* outputs, uintptr_t alignMask, Params* p) {
  if (!inputs || !outputs) return false;
  for (int r = 0; r < n; r++) {
    if (!inputs[r] || !outputs[r]) return false;
    if (((uintptr_t)inputs[r] | (uintptr_t)outputs[r]) & alignMask) return false;
    p->in[r] = (const char*)inputs[r];
    p->out[r] = (char*)outputs[r];
  }
  return true;
}

// The n outputs of a reduction: each non-null and element-aligned, stored into out[].
bool takeOutputs(int n, void* const* outputs, uint64_t esz, char** out) {
  if (!outputs) return false;
  for (int r = 0; r < n; r++) {
    if (!outputs[r] || ((uintptr_t)outputs[r] & (esz - 1))) return false;
    out[r] = (char*)outputs[r];
  }
  return true;
}

// The broadcast's outputs: each non-null; one that is the input itself is not written and stays null in out[].
// *any: some output is written.
template <typename T>
bool takeBroadcastOutputs(int n, const void* input, void* const* outputs, T** out, bool* any) {
  if (!input || !outputs) return false;
  *any = false;
  for (int r = 0; r < n; r++) {
    if (!outputs[r]) return false;
    out[r] = outputs[r] != input ? (T*)outputs[r] : nullptr;
    *any = *any || out[r];
  }
  return true;
}

// The parts tile [0, nElts): ascending, gapless, from 0, none empty, each from a pack boundary (epp elements per
// pack). `extra` is the part type's own condition.
template <typename Part, typename Extra>
bool partsTile(const Part* parts, int nParts, uint64_t nElts, uint64_t epp, Extra&& extra) {
  if (nParts < 0 || (nParts > 0 && !parts)) return false;
  uint64_t at = 0;
  for (int k = 0; k < nParts; k++) {
    const Part& q = parts[k];
    if (q.offset != at || q.count == 0 || q.count > nElts - at) return false;
    if (q.offset % epp || !extra(q)) return false;
    at += q.count;
  }
  return at == nElts;
}

// The grid of every launch below: a wave per item, four waves per workgroup, at least `least` (0 or 1) and at most
// `cap` workgroups, then maxWorkgroups where it is set. Beyond the grid the waves stride.
unsigned waveGrid(uint64_t items, uint64_t cap, uint64_t least, uint64_t maxWorkgroups) {
  uint64_t grid = std::min<uint64_t>(std::max<uint64_t>((items + kBlock / 64 - 1) / (kBlock / 64), least), cap);
  if (maxWorkgroups > 0 && grid > maxWorkgroups) grid = maxWorkgroups;
  return (unsigned)grid;
}

// The fill launch that carries a table of T by value: its block, the block's payload array, its launch function.
template <typename T>
struct FillOf;
template <>
struct FillOf<nexrFlatPart> {
  using Block = FlatPartsFill;
  static constexpr auto payload = &FlatPartsFill::parts;
  static constexpr auto launch = &launch_flat_parts;
};
template <>
struct FillOf<nexrFlatTreePart> {
  using Block = FlatTreePartsFill;
  static constexpr auto payload = &FlatTreePartsFill::parts;
  static constexpr auto launch = &launch_flat_tree_parts;
};
template <>
struct FillOf<uint64_t> {
  using Block = FlatGroupFill;
  static constexpr auto payload = &FlatGroupFill::words;
  static constexpr auto launch = &launch_flat_group_fill;
};

// A table too long for a launch's arguments, in a stream-ordered workspace: it travels by value in short launches
// ahead of the one, so nothing is read after return. The caller frees *ws behind its launch.
template <typename T>
nexrResult_t stageByValue(const T* src, size_t n, hipStream_t s, T** ws) {
  using Fill = FillOf<T>;
  NEXR_HIP(hipMallocAsync((void**)ws, n * sizeof(T), s));
  typename Fill::Block f;
  constexpr size_t cap = sizeof(f.*Fill::payload) / sizeof(T);
  for (size_t k = 0; k < n; k += cap) {
    f.dst = *ws + k;
    f.n = (int)std::min(cap, n - k);
    f.pad = 0;
    memcpy(f.*Fill::payload, src + k, (size_t)f.n * sizeof(T));
    const hipError_t e = Fill::launch(f, s);
    if (e != hipSuccess) {
      (void)hipFreeAsync(*ws, s);
      *ws = nullptr;
      return hipFail(e);
    }
  }
  return nexrSuccess;
}

// One launch with its table of n entries: in the argument block (`inl`) where at most inlineN of them do, else
// staged and named by *ext; then the launch, the workspace's free behind it, and the launch's error.
template <typename T, typename Ext, typename Launch>
nexrResult_t launchWithTable(const T* src, size_t n, size_t inlineN, void* inl, Ext* ext, hipStream_t s,
                             Launch&& launch) {
  T* ws = nullptr;
  if (n > inlineN) {
    const nexrResult_t res = stageByValue(src, n, s, &ws);
    if (res != nexrSuccess) return res;
    *ext = (Ext)ws;
  } else if (n) {
    memcpy(inl, src, n * sizeof(T));
  }
  const hipError_t e = launch();
  if (ws) (void)hipFreeAsync(ws, s);
  NEXR_HIP(e);
  return nexrSuccess;
}

// A checked call as one value: the result of the checks, the dispatch after the semantics, the launch's parameters
// over the pointers as given, and the caller's parts (read again at the launch).
template <typename Params, typename Part>
struct Checked {
  nexrResult_t res = nexrInvalidArgument;
  int dt = 0, op = 0;
  const Part* parts = nullptr;
  Params p;
};
using FlatCall = Checked<FlatParams, nexrFlatPart>;
using FlatTreeCall = Checked<FlatTreeParams, nexrFlatTreePart>;

// The per-rank kernels' block from the plain one: the fields the ring's and the tree's blocks share by name.
template <typename From, typename To>
void preMulFrom(const From& p, const uint64_t* scalars, int arePtrs, To* q) {
  memset((void*)q, 0, sizeof(*q));
  memcpy(q->in, p.in, sizeof(q->in));
  memcpy(q->out, p.out, sizeof(q->out));
  memcpy(q->scalars, scalars, (size_t)p.nRanks * sizeof(uint64_t));
  q->winBeg = p.winBeg;
  q->winEnd = p.winEnd;
  q->nRanks = p.nRanks;
  q->userFirst = p.userFirst;
  q->preOp = p.preOp;
  q->postOp = p.postOp;
  q->nParts = p.nParts;
  q->nOut = p.nOut;
  q->scalarsArePtrs = arePtrs ? 1 : 0;
}
}  // namespace

// The ownership plan of nexrSymAllReduce from rank 0's pointers (include/nexr.h; reference
// src/device/symmetric/all_reduce.hh:199-252): the two passes' piece counts and where the ends lie.
static void symPlan(uintptr_t in0, uintptr_t out0, uint64_t nElts, uint64_t esz, uint64_t nRanksBlocks,
                    nexr::SymParams* p) {
  const uint64_t nBytes = nElts * esz;
  const uint64_t pre = std::min<uint64_t>((16u - in0) % 16u, nBytes);  // nPreBytes (:207-208)
  const uint64_t d = (in0 - out0) % 16u;
  uint64_t cursor = pre;
  p->p1Off = cursor;
  p->p1Pieces = 0;
  if (d == 0) {  // 16-byte packs: chunks of 4 warps x 4 packs x 32 lanes (:213-228)
    uint64_t chunks = (nBytes - cursor) / 8192;
    chunks -= chunks % nRanksBlocks;
    p->p1Pieces = chunks * 4;
    cursor += chunks * 8192;
  }
  p->p2Off = cursor;
  p->p2Pieces = 0;
  if (esz == 4 || d % 4 == 0) {  // 4-byte packs (:230-245)
    uint64_t chunks = (nBytes - cursor) / 2048;
    chunks -= chunks % nRanksBlocks;
    p->p2Pieces = chunks * 4;
    cursor += chunks * 2048;
  }
  p->preElts = pre / esz;  // the ends (:249-251): nPreElts, then nSufElts from the cursor
  p->sufOff = cursor;
  p->nEnds = p->preElts + (nBytes - cursor) / esz;
}

NEXR_API nexrResult_t nexrSymAllReduce(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                       int datatype, int devRedOp, uint64_t redOpArg, int nBlocks,
                                       nexrStream_t stream) {
  (void)redOpArg;
  if (!flatRanksOk(nRanks) || nBlocks < 0 || nBlocks > 64) return nexrInvalidArgument;
  if (datatype != nexrFloat32 && datatype != nexrFloat16 && datatype != nexrBfloat16) return nexrInvalidArgument;
  if (devRedOp != nexrDevSum) return nexrInvalidArgument;
  const uint64_t esz = typeSize(datatype);
  SymParams p;
  memset(&p, 0, sizeof(p));
  if (!takeBuffers(nRanks, inputs, outputs, esz - 1, &p)) return nexrInvalidArgument;
  if (nElts > (size_t)-1 / esz) return nexrInvalidArgument;
  if (nElts == 0) return nexrSuccess;
  symPlan((uintptr_t)inputs[0], (uintptr_t)outputs[0], nElts, esz, (uint64_t)nRanks * (uint64_t)(nBlocks ? nBlocks : 1),
          &p);
  p.nRanks = nRanks;
  p.nFold = semantics() == nexrSemanticsShipped ? 1 : nRanks;  // SKIP_COMP: every add returns its first operand
  // One-shot: a wave per piece or group of 32 end elements; beyond the cap the kernel strides.
  const uint64_t items = p.p1Pieces + p.p2Pieces + (p.nEnds + 31) / 32;
  NEXR_HIP(launch_sym_all_reduce(datatype, p, waveGrid(items, gridCap(kBlock), 0, 0), (hipStream_t)stream));
  return nexrSuccess;
}

// The one-shot grid of the symmetric reduce-scatter and all-gather: every chunk of chunkBytes is whole
// 2048-byte pieces, groups of 64 16-byte packs and one tail item; a wave per item and rank; beyond the cap the
// kernels stride. maxGrid > 0 caps it (the host forms, hostGrid).
static unsigned symChunkGrid(uint64_t chunkBytes, uint64_t esz, int nRanks, uint64_t maxGrid = 0) {
  const uint64_t rem = chunkBytes % 2048;
  const uint64_t perRank = chunkBytes / 2048 + (rem / 16 + 63) / 64 + (rem % 16 / esz ? 1 : 0);
  return waveGrid(perRank * (uint64_t)nRanks, gridCap(kBlock), 0, maxGrid);
}

NEXR_API nexrResult_t nexrSymReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                           size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                           nexrStream_t stream) {
  (void)redOpArg;
  if (!flatRanksOk(nRanks)) return nexrInvalidArgument;
  if (datatype != nexrFloat32 && datatype != nexrFloat16 && datatype != nexrBfloat16) return nexrInvalidArgument;
  if (devRedOp != nexrDevSum) return nexrInvalidArgument;
  const uint64_t esz = typeSize(datatype);
  SymRsParams p;
  memset(&p, 0, sizeof(p));
  if (!takeBuffers(nRanks, inputs, outputs, esz - 1, &p)) return nexrInvalidArgument;
  if (nElts > (size_t)-1 / esz / (size_t)nRanks) return nexrInvalidArgument;  // an input's nRanks * nElts * esz bytes
  if (nElts == 0) return nexrSuccess;
  p.chunkBytes = (uint64_t)nElts * esz;
  p.nRanks = nRanks;
  p.nFold = semantics() == nexrSemanticsShipped ? 1 : nRanks;  // SKIP_COMP: every add returns its first operand
  NEXR_HIP(launch_sym_reduce_scatter(datatype, p, symChunkGrid(p.chunkBytes, esz, nRanks), (hipStream_t)stream));
  return nexrSuccess;
}

namespace {
// The reference's inPlace, per rank.
uint64_t symInPlace(const SymAgParams& p, int nRanks, size_t nBytes) {
  uint64_t bits = 0;
  for (int r = 0; r < nRanks; r++)
    if ((uintptr_t)p.in[r] == (uintptr_t)p.out[r] + (uintptr_t)r * nBytes) bits |= 1ull << r;
  return bits;
}
}  // namespace

NEXR_API nexrResult_t nexrSymAllGather(int nRanks, const void* const* inputs, void* const* outputs, size_t nBytes,
                                       nexrStream_t stream) {
  if (!flatRanksOk(nRanks)) return nexrInvalidArgument;
  if (nBytes > (size_t)-1 / (size_t)nRanks) return nexrInvalidArgument;  // an output's nRanks * nBytes bytes
  SymAgParams p;
  memset(&p, 0, sizeof(p));
  if (!takeBuffers(nRanks, inputs, outputs, 0, &p)) return nexrInvalidArgument;
  if (nBytes == 0) return nexrSuccess;
  p.inPlace = symInPlace(p, nRanks, nBytes);
  p.nBytes = nBytes;
  p.nRanks = nRanks;
  NEXR_HIP(launch_sym_all_gather(p, symChunkGrid(nBytes, 1, nRanks), (hipStream_t)stream));
  return nexrSuccess;
}

// ---- nexrFlatAllReduce, nexrFlatReduceScatter, nexrFlatReduce -----------------------------------------------
// The checks the three share, then what the semantics make of the call (as simpleStepsGroup hands them to
// launch_simple_group: fork changes the dispatch type; shipped folds nothing, and what survives is the first
// operand of the chain's last step).
namespace {
// The rank count, datatype and op that a flat reduction takes.
nexrResult_t flatOpCheck(int nRanks, int datatype, int devRedOp, uint64_t redOpArg) {
  if (!flatRanksOk(nRanks)) return nexrInvalidArgument;
  return typeOpOk(datatype, devRedOp, redOpArg) ? nexrSuccess : nexrInvalidArgument;
}

// What the semantics make of a checked call: the dispatch and the fields that flat_fold reads (FlatParams' names).
struct FlatSemantics {
  int dt, op, nFold, shift, preOp, postOp;
};
FlatSemantics flatSemantics(int nRanks, int datatype, int devRedOp, int userFirst) {
  int srcIsInput = 1, postOp = 1, firstWins = 0;
  FlatSemantics m;
  m.dt = datatype;
  m.op = devRedOp;
  llSemantics(&m.dt, &m.op, &srcIsInput, &postOp, &firstWins);
  m.nFold = firstWins ? 1 : nRanks;
  m.shift = firstWins && userFirst ? nRanks - 1 : 0;
  m.preOp = srcIsInput;
  m.postOp = postOp;
  return m;
}

// c->p zeroed, then the inputs and what the semantics make of the call. False: an argument is refused.
bool flatPrepare(int nRanks, const void* const* inputs, int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                 FlatCall* c) {
  if (!inputs || flatOpCheck(nRanks, datatype, devRedOp, redOpArg) != nexrSuccess) return false;
  const uint64_t esz = typeSize(datatype);
  FlatParams& p = c->p;
  memset((void*)&p, 0, sizeof(p));
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || ((uintptr_t)inputs[r] & (esz - 1))) return false;
    p.in[r] = (const char*)inputs[r];
  }
  const FlatSemantics m = flatSemantics(nRanks, datatype, devRedOp, userFirst);
  c->dt = m.dt;
  c->op = m.op;
  p.nRanks = nRanks;
  p.redArg = redOpArg;
  p.userFirst = userFirst ? 1 : 0;
  p.nFold = m.nFold;
  p.shift = m.shift;
  p.preOp = m.preOp;
  p.postOp = m.postOp;
  return true;
}

// One-shot: a wave per 2048-byte piece of every region; maxGrid > 0 caps the grid (the host forms, hostGrid).
unsigned flatGrid(uint64_t regionBytes, int nRegions, uint64_t maxGrid = 0) {
  return waveGrid((regionBytes + 2047) / 2048 * (uint64_t)nRegions, gridCap(kBlock), 0, maxGrid);
}

// The checks of nexrFlatAllReduce, and the launch's parameters over the pointers as given (no device call).
FlatCall flatAllReduceCheck(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts, int datatype,
                            int devRedOp, uint64_t redOpArg, int userFirst, const nexrFlatPart* parts, int nParts) {
  FlatCall c;
  FlatParams& p = c.p;
  if (!flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &c)) return c;
  const uint64_t esz = typeSize(datatype), epp = 16 / esz;
  if (!takeOutputs(nRanks, outputs, esz, p.out)) return c;
  if (nElts > (size_t)-1 / esz) return c;
  const bool tiled = partsTile(parts, nParts, nElts, epp, [&](const nexrFlatPart& q) {
    return q.chunkCount != 0 && q.chunkCount % epp == 0 && q.chunkCount <= (uint64_t)-1 / (uint64_t)nRanks;
  });
  if (!tiled) return c;
  p.coll = kFlatAllReduce;
  p.regionBytes = p.winEnd = (uint64_t)nElts * esz;
  p.nParts = nParts;
  p.nOut = nRanks;
  c.parts = parts;
  c.res = nexrSuccess;
  return c;
}

FlatCall flatReduceScatterCheck(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                int datatype, int devRedOp, uint64_t redOpArg, int userFirst) {
  FlatCall c;
  FlatParams& p = c.p;
  if (!flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &c)) return c;
  const uint64_t esz = typeSize(datatype);
  if (!takeOutputs(nRanks, outputs, esz, p.out)) return c;
  if (nElts > (size_t)-1 / esz / (size_t)nRanks) return c;  // an input's nRanks * nElts * esz bytes
  p.coll = kFlatReduceScatter;
  p.regionBytes = p.winEnd = (uint64_t)nElts * esz;
  c.res = nexrSuccess;
  return c;
}

FlatCall flatReduceCheck(int nRanks, const void* const* inputs, void* output, int root, size_t nElts, int datatype,
                         int devRedOp, uint64_t redOpArg, int userFirst) {
  FlatCall c;
  FlatParams& p = c.p;
  if (!output || !flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &c)) return c;
  const uint64_t esz = typeSize(datatype);
  if (root < 0 || root >= nRanks || ((uintptr_t)output & (esz - 1))) return c;
  if (nElts > (size_t)-1 / esz) return c;
  p.out[root] = (char*)output;
  p.root = root;
  p.coll = kFlatReduce;
  p.regionBytes = p.winEnd = (uint64_t)nElts * esz;
  c.res = nexrSuccess;
  return c;
}

// The one place that knows how a checked ring call is launched, over the window that c.p holds: a region per rank
// for the reduce-scatter and one otherwise, the all-reduce's parts as the launch's table, and with scalars the
// per-rank kernel, unless the semantics turned the op away from PreMulSum (shipped: a bit copy without a pre-op,
// the plain kernel's launch, and no scalar is read). maxGrid > 0 caps the grid.
nexrResult_t flatLaunch(FlatCall& c, const uint64_t* scalars, int arePtrs, uint64_t maxGrid, hipStream_t s) {
  FlatParams& p = c.p;
  const unsigned grid = flatGrid(p.winEnd - p.winBeg, p.coll == kFlatReduceScatter ? p.nRanks : 1, maxGrid);
  if (!scalars || c.op != nexrDevPreMulSum)
    return launchWithTable(c.parts, (size_t)p.nParts, (size_t)kFlatInlineParts, p.parts, &p.ext, s,
                           [&] { return launch_flat(c.dt, c.op, p, grid, s); });
  FlatPreMulParams q;
  preMulFrom(p, scalars, arePtrs, &q);
  q.regionBytes = p.regionBytes;
  q.coll = p.coll;
  q.nFold = p.nFold;
  q.shift = p.shift;
  q.root = p.root;
  return launchWithTable(c.parts, (size_t)p.nParts, (size_t)kFlatPreMulInlineParts, q.parts, &q.ext, s,
                         [&] { return launch_flat_premul(c.dt, q, grid, s); });
}
}  // namespace

NEXR_API nexrResult_t nexrFlatAllReduce(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                        int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                        const nexrFlatPart* parts, int nParts, nexrStream_t stream) {
  FlatCall c = flatAllReduceCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst, parts,
                                  nParts);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatLaunch(c, nullptr, 0, 0, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrFlatReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, nexrStream_t stream) {
  FlatCall c = flatReduceScatterCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatLaunch(c, nullptr, 0, 0, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrFlatReduce(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                                     int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                     nexrStream_t stream) {
  FlatCall c = flatReduceCheck(nRanks, inputs, output, root, nElts, datatype, devRedOp, redOpArg, userFirst);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatLaunch(c, nullptr, 0, 0, (hipStream_t)stream);
}

// ---- nexrFlatTreeAllReduce, nexrFlatBroadcast ---------------------------------------------------------------
namespace {
// One tree's links as a program (include/nexr.h): from the root, down[0]'s value first, then the rank's own
// input, then for every further child PUSH, the child, MERGE. `need` is the most values alive at once (the
// accumulator and the saved ones). False: the links are not one spanning tree with packed children.
bool flatTreeCompile(const nexrFlatTreeLinks* links, int n, std::vector<uint8_t>* code, int* need, int* root) {
  int nRoots = 0, slots = 0;
  *root = -1;
  for (int r = 0; r < n; r++) {
    const nexrFlatTreeLinks& l = links[r];
    if (l.up < -1 || l.up >= n || l.up == r) return false;
    if (l.up == -1) {
      nRoots++;
      *root = r;
    } else {  // every up matched by its parent's down, once
      const nexrFlatTreeLinks& p = links[l.up];
      if ((p.down[0] == r) + (p.down[1] == r) + (p.down[2] == r) != 1) return false;
    }
    bool ended = false;
    for (int k = 0; k < 3; k++) {
      const int d = l.down[k];
      if (d < -1 || d >= n) return false;
      if (d == -1) {
        ended = true;
        continue;
      }
      if (ended || links[d].up != r) return false;  // packed first; every down matched by its child's up
      slots++;
    }
  }
  // one parent each and n - 1 child slots, every one its child's up: every rank but the root is some rank's
  // child exactly once
  if (nRoots != 1 || slots != n - 1) return false;
  code->clear();
  int depth = 0, most = 1;
  // iterative walk: (rank, next child) frames; a rank has one parent, so what the root reaches is a tree
  std::vector<std::pair<int, int>> stack{{*root, 0}};
  int seen = 0;
  while (!stack.empty()) {
    const int r = stack.back().first, k = stack.back().second;
    const nexrFlatTreeLinks& l = links[r];
    const int nd = l.down[0] < 0 ? 0 : l.down[1] < 0 ? 1 : l.down[2] < 0 ? 2 : 3;
    if (nd == 0) {
      code->push_back((uint8_t)(kFlatTreeLeaf << 6 | r));
      seen++;
      stack.pop_back();
      continue;
    }
    if (k == 1) {  // behind down[0]
      code->push_back((uint8_t)(kFlatTreeJoin << 6 | r));
      seen++;
    } else if (k > 1) {  // behind a further child
      code->push_back((uint8_t)(kFlatTreeMerge << 6));
      depth--;
    }
    if (k == nd) {
      stack.pop_back();
      continue;
    }
    if (k >= 1) {
      code->push_back((uint8_t)(kFlatTreePush << 6));
      depth++;
      most = std::max(most, depth + 1);
    }
    stack.back().second = k + 1;
    stack.push_back({l.down[k], 0});
  }
  if (seen != n) return false;  // ranks the root does not reach: a cycle among them
  *need = most;
  return true;
}

FlatTreeCall flatTreeCheck(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts, int datatype,
                           int devRedOp, uint64_t redOpArg, int userFirst, const nexrFlatTreeLinks* const* trees,
                           int nTrees, const nexrFlatTreePart* parts, int nParts) {
  FlatTreeCall c;
  FlatTreeParams& p = c.p;
  FlatCall f;  // the shared checks and what the semantics make of the call
  if (!flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &f)) return c;
  const FlatParams& fp = f.p;
  const uint64_t esz = typeSize(datatype), epp = 16 / esz;
  memset((void*)&p, 0, sizeof(p));
  memcpy(p.in, fp.in, sizeof(p.in));
  if (!takeOutputs(nRanks, outputs, esz, p.out)) return c;
  if (nElts > (size_t)-1 / esz) return c;
  if (!trees || nTrees < 1 || nTrees > 2) return c;
  const bool firstWins = fp.nFold == 1;
  for (int t = 0; t < nTrees; t++) {
    if (!trees[t]) return c;
    std::vector<uint8_t> code;
    int need = 0, root = -1;
    if (!flatTreeCompile(trees[t], nRanks, &code, &need, &root)) return c;
    if (need > kFlatTreeSlots || code.size() > (size_t)kFlatTreeProgBytes) return c;
    if (firstWins) {  // every reduce returns its first operand: one rank's input survives
      int r = root;
      if (!userFirst)
        while (trees[t][r].down[0] >= 0) {  // the peer is first, the last child's last
          const nexrFlatTreeLinks& l = trees[t][r];
          r = l.down[2] >= 0 ? l.down[2] : l.down[1] >= 0 ? l.down[1] : l.down[0];
        }
      code.assign(1, (uint8_t)(kFlatTreeLeaf << 6 | r));
    }
    uint8_t order[NEXR_SYM_MAX_RANKS] = {0};
    int nIn = 0;
    for (uint8_t ins : code)
      if ((ins >> 6) <= kFlatTreeJoin) order[nIn++] = ins & 63;
    FlatTreeProgram& g = p.prog[t];
    memcpy(g.code, code.data(), code.size());
    memcpy(g.order, order, sizeof(order));
    g.nCode = (int)code.size();
    g.nIn = nIn;
  }
  if (!partsTile(parts, nParts, nElts, epp, [&](const nexrFlatTreePart& q) { return q.tree < (uint32_t)nTrees; }))
    return c;
  p.nBytes = p.winEnd = (uint64_t)nElts * esz;
  p.redArg = fp.redArg;
  p.nRanks = p.nOut = nRanks;
  p.userFirst = fp.userFirst;
  p.preOp = fp.preOp;
  p.postOp = fp.postOp;
  p.nParts = nParts;
  c.dt = f.dt;
  c.op = f.op;
  c.parts = parts;
  c.res = nexrSuccess;
  return c;
}

// flatLaunch for a checked tree all-reduce.
nexrResult_t flatTreeLaunch(FlatTreeCall& c, const uint64_t* scalars, int arePtrs, uint64_t maxGrid, hipStream_t s) {
  FlatTreeParams& p = c.p;
  const unsigned grid = flatGrid(p.winEnd - p.winBeg, 1, maxGrid);
  if (!scalars || c.op != nexrDevPreMulSum)
    return launchWithTable(c.parts, (size_t)p.nParts, (size_t)kFlatTreeInlineParts, p.parts, &p.ext, s,
                           [&] { return launch_flat_tree(c.dt, c.op, p, grid, s); });
  FlatTreePreMulParams q;
  preMulFrom(p, scalars, arePtrs, &q);
  q.nBytes = p.nBytes;
  q.prog[0] = p.prog[0];
  q.prog[1] = p.prog[1];
  return launchWithTable(c.parts, (size_t)p.nParts, (size_t)kFlatTreePreMulInlineParts, q.parts, &q.ext, s,
                         [&] { return launch_flat_tree_premul(c.dt, q, grid, s); });
}
}  // namespace

NEXR_API nexrResult_t nexrFlatTreeAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, const nexrFlatTreeLinks* const* trees, int nTrees,
                                            const nexrFlatTreePart* parts, int nParts, nexrStream_t stream) {
  FlatTreeCall c = flatTreeCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst, trees,
                                 nTrees, parts, nParts);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatTreeLaunch(c, nullptr, 0, 0, (hipStream_t)stream);
}

// ---- nexrFlat*PreMul: PreMulSum with a scalar per rank --------------------------------------------------------
// The plain entry's checks run with nexrDevPreMulSum and make the plain launch's parameters; the scalars are
// checked; the launch (flatLaunch, flatTreeLaunch) moves the fields into the per-rank kernels' block.
namespace {
nexrResult_t flatScalarsCheck(int nRanks, const uint64_t* scalars, int arePtrs, int datatype) {
  if (!scalars) return nexrInvalidArgument;
  const uint64_t esz = typeSize(datatype);
  for (int r = 0; arePtrs && r < nRanks; r++)
    if (!scalars[r] || (scalars[r] & (esz - 1))) return nexrInvalidArgument;
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatAllReducePreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                              size_t nElts, int datatype, const uint64_t* scalars,
                                              int scalarsArePtrs, int userFirst, const nexrFlatPart* parts,
                                              int nParts, nexrStream_t stream) {
  FlatCall c = flatAllReduceCheck(nRanks, inputs, outputs, nElts, datatype, nexrDevPreMulSum, 0, userFirst, parts,
                                  nParts);
  if (c.res == nexrSuccess) c.res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatLaunch(c, scalars, scalarsArePtrs, 0, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrFlatReduceScatterPreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                                  size_t nElts, int datatype, const uint64_t* scalars,
                                                  int scalarsArePtrs, int userFirst, nexrStream_t stream) {
  FlatCall c = flatReduceScatterCheck(nRanks, inputs, outputs, nElts, datatype, nexrDevPreMulSum, 0, userFirst);
  if (c.res == nexrSuccess) c.res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatLaunch(c, scalars, scalarsArePtrs, 0, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrFlatReducePreMul(int nRanks, const void* const* inputs, void* output, int root,
                                           size_t nElts, int datatype, const uint64_t* scalars, int scalarsArePtrs,
                                           int userFirst, nexrStream_t stream) {
  FlatCall c = flatReduceCheck(nRanks, inputs, output, root, nElts, datatype, nexrDevPreMulSum, 0, userFirst);
  if (c.res == nexrSuccess) c.res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatLaunch(c, scalars, scalarsArePtrs, 0, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrFlatTreeAllReducePreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                                  size_t nElts, int datatype, const uint64_t* scalars,
                                                  int scalarsArePtrs, int userFirst,
                                                  const nexrFlatTreeLinks* const* trees, int nTrees,
                                                  const nexrFlatTreePart* parts, int nParts, nexrStream_t stream) {
  FlatTreeCall c = flatTreeCheck(nRanks, inputs, outputs, nElts, datatype, nexrDevPreMulSum, 0, userFirst, trees,
                                 nTrees, parts, nParts);
  if (c.res == nexrSuccess) c.res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  return flatTreeLaunch(c, scalars, scalarsArePtrs, 0, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrFlatBroadcast(int nRanks, const void* input, void* const* outputs, size_t nBytes,
                                        nexrStream_t stream) {
  if (!flatRanksOk(nRanks)) return nexrInvalidArgument;
  FlatBcastParams p;
  memset((void*)&p, 0, sizeof(p));
  bool any = false;
  if (!takeBroadcastOutputs(nRanks, input, outputs, p.out, &any)) return nexrInvalidArgument;
  if (nBytes == 0 || !any) return nexrSuccess;
  p.in = (const char*)input;
  p.nBytes = p.winEnd = nBytes;
  p.nRanks = nRanks;
  NEXR_HIP(launch_flat_bcast(p, flatGrid(nBytes, 1), (hipStream_t)stream));
  return nexrSuccess;
}

// ---- nexrFlatAllToAll -------------------------------------------------------------------------------------------
// Every check before any device call; the ranges are half-open, as nexrFlatGroupPlan compares them. The host
// picks the instance: packs where no pack can straddle two blocks (nBytes % 16 == 0), bytes otherwise.
NEXR_API nexrResult_t nexrFlatAllToAll(int nRanks, const void* const* inputs, void* const* outputs, size_t nBytes,
                                       int maxWorkgroups, nexrStream_t stream) {
  if (maxWorkgroups < 0 || !flatRanksOk(nRanks)) return nexrInvalidArgument;
  if (nBytes > (size_t)-1 / (size_t)nRanks) return nexrInvalidArgument;  // a buffer's nRanks * nBytes bytes
  const uintptr_t row = (uintptr_t)nRanks * nBytes;
  FlatAllToAllParams p;
  memset((void*)&p, 0, sizeof(p));
  if (!takeBuffers(nRanks, inputs, outputs, 0, &p)) return nexrInvalidArgument;
  if (!nexr_exchange_v::fixedRangesOk(nRanks, inputs, outputs, row, row, true)) return nexrInvalidArgument;
  if (nBytes == 0) return nexrSuccess;
  const bool bytes = (nBytes & 15u) != 0;
  p.blockBytes = nBytes;
  p.nRanks = nRanks;
  p.piecesPer = ((bytes ? (uint64_t)nBytes : (uint64_t)row) + 2047) / 2048;
  p.nItems = p.piecesPer * (uint64_t)nRanks * (bytes ? (uint64_t)nRanks : 1);
  const unsigned grid = waveGrid(p.nItems, gridCap(kBlock), 0, (uint64_t)maxWorkgroups);
  NEXR_HIP(launch_flat_alltoall(p, bytes, grid, (hipStream_t)stream));
  return nexrSuccess;
}

// ---- nexrFlatAllToAll2D, nexrFlatAllGather2D ----------------------------------------------------------------------
namespace {
// Every check before any device call, then the launch. A side's two strides follow from its layout; the gather is
// the exchange whose source has no block stride and the input's own row pitch, written rows out. The host picks the
// access width so that no unit can straddle two block rows.
nexrResult_t flatPitched(int nRanks, const void* const* inputs, void* const* outputs, size_t rows, size_t nBytes,
                         int inLayout, int outLayout, bool gather, int maxWorkgroups, nexrStream_t stream) {
  if (maxWorkgroups < 0 || !flatRanksOk(nRanks)) return nexrInvalidArgument;
  if ((inLayout != nexrLayoutBlocks && inLayout != nexrLayoutRows) ||
      (outLayout != nexrLayoutBlocks && outLayout != nexrLayoutRows))
    return nexrInvalidArgument;
  if (rows > (size_t)0x7fffffff) return nexrInvalidArgument;
  const size_t n = (size_t)nRanks;
  if (rows && nBytes > (size_t)-1 / n / rows) return nexrInvalidArgument;  // a buffer's n * rows * nBytes bytes
  const uintptr_t outLen = (uintptr_t)(n * rows * nBytes), inLen = gather ? (uintptr_t)(rows * nBytes) : outLen;
  FlatPitchedParams p;
  memset((void*)&p, 0, sizeof(p));
  if (!takeBuffers(nRanks, inputs, outputs, 0, &p)) return nexrInvalidArgument;
  if (!nexr_exchange_v::fixedRangesOk(nRanks, inputs, outputs, inLen, outLen, true)) return nexrInvalidArgument;
  if (outLen == 0) return nexrSuccess;
  if (!gather && (rows == 1 || (inLayout == nexrLayoutBlocks && outLayout == nexrLayoutBlocks)))
    return nexrFlatAllToAll(nRanks, inputs, outputs, rows * nBytes, maxWorkgroups, stream);
  const uint64_t B = nBytes;
  const int width = (B & 15u) == 0 ? 16 : (B & 3u) == 0 ? 4 : 1;
  p.runBytes = B;
  p.inBlock = gather ? 0 : inLayout == nexrLayoutBlocks ? (uint64_t)rows * B : B;
  p.inPitch = gather || inLayout == nexrLayoutBlocks ? B : (uint64_t)n * B;
  p.outBlock = outLayout == nexrLayoutBlocks ? (uint64_t)rows * B : B;
  p.outPitch = outLayout == nexrLayoutBlocks ? B : (uint64_t)n * B;
  p.inner = outLayout == nexrLayoutBlocks ? (uint32_t)rows : (uint32_t)n;
  p.outBytes = outLen;
  p.nRuns = (uint64_t)n * rows;
  p.nRanks = nRanks;
  const uint64_t piece = (uint64_t)128 * (uint64_t)width;
  p.piecesPer = p.outBytes / piece + (p.outBytes % piece ? 1 : 0);
  p.nItems = p.piecesPer * (uint64_t)n;
  const unsigned grid = waveGrid(p.nItems, gridCap(kBlock), 0, (uint64_t)maxWorkgroups);
  NEXR_HIP(launch_flat_pitched(p, width, grid, (hipStream_t)stream));
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatAllToAll2D(int nRanks, const void* const* inputs, void* const* outputs, size_t rows,
                                         size_t nBytes, int inLayout, int outLayout, int maxWorkgroups,
                                         nexrStream_t stream) {
  return flatPitched(nRanks, inputs, outputs, rows, nBytes, inLayout, outLayout, false, maxWorkgroups, stream);
}

NEXR_API nexrResult_t nexrFlatAllGather2D(int nRanks, const void* const* inputs, void* const* outputs, size_t rows,
                                          size_t nBytes, int maxWorkgroups, nexrStream_t stream) {
  return flatPitched(nRanks, inputs, outputs, rows, nBytes, nexrLayoutRows, nexrLayoutRows, true, maxWorkgroups,
                     stream);
}

// ---- nexrFlatAllToAllv ------------------------------------------------------------------------------------------
namespace {
// Workgroups of flat_exchange_v_kernel the current device keeps resident, the default cap of its grid: per CU eight
// (what the kernel's registers admit at 256 threads), or as many as find their 16 * n * n bytes of LDS in a CU's
// 160 KiB where that is fewer (36 ranks and more: two at 64). 2,048 on the 256 CUs of an MI355X up to 35 ranks, which
// is what DESIGN 8.13 measured; nothing above 16 ranks has been measured.
// n == 0: a kernel without LDS (nexr_flat_scatter_v.hip), eight per CU at any rank count.
nexrResult_t flatExchangeVResident(int n, uint64_t* resident) {
  constexpr int kDevs = 16;
  static std::atomic<int> cusOf[kDevs];
  int dev = 0;
  NEXR_HIP(hipGetDevice(&dev));
  const bool cached = dev >= 0 && dev < kDevs;
  int cus = cached ? cusOf[dev].load(std::memory_order_relaxed) : 0;
  if (cus <= 0) {
    NEXR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cached && cus > 0) cusOf[dev].store(cus, std::memory_order_relaxed);
  }
  const uint64_t perCu = n ? std::min<uint64_t>(8, (uint64_t)(160 << 10) / ((uint64_t)16 * n * n)) : 8;
  *resident = std::max<uint64_t>(perCu * (uint64_t)std::max(cus, 1), 1);
  return nexrSuccess;
}

// The grid of the counted launches: waveGrid up to the workgroups the device keeps resident (ldsRanks: what
// flatExchangeVResident takes), so that a workgroup's prologue serves many pieces and not four. Device counts with
// no capacity at all still launch one workgroup: the verdict is the kernel's.
nexrResult_t flatCountedGrid(int ldsRanks, uint64_t items, int maxWorkgroups, unsigned* grid) {
  uint64_t resident = 0;
  const nexrResult_t res = flatExchangeVResident(ldsRanks, &resident);
  if (res != nexrSuccess) return res;
  *grid = waveGrid(items, resident, 1, (uint64_t)maxWorkgroups);
  return nexrSuccess;
}

// What the counted entries share once the rank count and the element size are checked: the arrays, the residence,
// device counts' alignment and status word, the capacities and ranges (countWords counts), and the fields that
// FlatExchangeVParams and FlatScatterVParams have in common. A buffer of no capacity may be null (buffersOk), so
// the pointers are not takeBuffers'.
template <typename Params>
nexrResult_t flatCountedPrelude(int n, const void* const* inputs, void* const* outputs, const uint64_t* counts,
                                int residence, size_t esz, const size_t* inElts, const size_t* outElts,
                                uint32_t* status, int maxWorkgroups, size_t countWords, Params* p) {
  if (!inputs || !outputs || !counts || !inElts || !outElts || maxWorkgroups < 0) return nexrInvalidArgument;
  if (residence != nexrScalarDevice && residence != nexrScalarHostImmediate) return nexrInvalidArgument;
  const bool dev = residence == nexrScalarDevice;
  if (dev && (!status || ((uintptr_t)counts & 7u))) return nexrInvalidArgument;
  if (!nexr_exchange_v::buffersOk(n, inputs, outputs, inElts, outElts, esz, counts, status, dev, countWords))
    return nexrInvalidArgument;
  for (int r = 0; r < n; r++) {
    p->in[r] = (const char*)inputs[r];
    p->out[r] = (char*)outputs[r];
    p->inElts[r] = inElts[r];
    p->outElts[r] = outElts[r];
  }
  p->status = status;
  p->nRanks = n;
  return nexrSuccess;
}

int eszShift(size_t esz) { return esz == 1 ? 0 : esz == 2 ? 1 : esz == 4 ? 2 : 3; }
}  // namespace

// Every check before any device call. Host counts are summed here and size the grid exactly; device counts are
// never read here, and the grid comes from the capacities (the kernel derives the true item count itself). Host
// counts of more than kFlatExchangeVInlineRanks ranks are the launch's staged table, as nexrFlatGroup's.
NEXR_API nexrResult_t nexrFlatAllToAllv(int nRanks, const void* const* inputs, void* const* outputs,
                                        const uint64_t* counts, int residence, size_t esz, const size_t* inElts,
                                        const size_t* outElts, uint32_t* status, int maxWorkgroups,
                                        nexrStream_t stream) {
  if (!flatRanksOk(nRanks) || !eszOk(esz)) return nexrInvalidArgument;
  const int n = nRanks;
  const bool dev = residence == nexrScalarDevice;
  FlatExchangeVParams p;
  memset((void*)&p, 0, sizeof(p));
  nexrResult_t res = flatCountedPrelude(n, inputs, outputs, counts, residence, esz, inElts, outElts, status,
                                        maxWorkgroups, (size_t)n * n, &p);
  if (res != nexrSuccess) return res;
  uint64_t items = 0;
  if (dev) {
    for (int d = 0; d < n; d++) items += ((uint64_t)outElts[d] * esz + 2047) / 2048;
  } else {
    uint64_t col[NEXR_SYM_MAX_RANKS];
    if (!nexr_exchange_v::countsFit(n, counts, inElts, outElts, col)) return nexrInvalidArgument;
    for (int d = 0; d < n; d++) items += (col[d] * esz + 2047) / 2048;
    if (items == 0) return nexrSuccess;
  }
  p.shift = eszShift(esz);
  unsigned grid = 0;
  res = flatCountedGrid(n, items, maxWorkgroups, &grid);
  if (res != nexrSuccess) return res;
  hipStream_t s = (hipStream_t)stream;
  const auto launch = [&] { return launch_flat_exchange_v(p, grid, s); };
  if (dev) {
    p.ext = counts;
    NEXR_HIP(launch());
    return nexrSuccess;
  }
  constexpr size_t inlineWords = (size_t)kFlatExchangeVInlineRanks * kFlatExchangeVInlineRanks;
  return launchWithTable(counts, (size_t)n * n, inlineWords, p.inl, &p.ext, s, launch);
}

// ---- nexrFlatReduceScatterv, nexrFlatAllGatherv -----------------------------------------------------------------
namespace {
// The checks the two share with nexrFlatAllToAllv (arrays, residence, capacities, ranges), the host counts' fit,
// and the launch's parameters but for what the reduction adds. *items: the 2048-byte pieces that size the grid,
// exact under host counts (0: nothing to do), those of the capacities under device counts.
nexrResult_t flatScatterVCheck(int n, const void* const* inputs, void* const* outputs, const uint64_t* counts,
                               int residence, size_t esz, const size_t* inElts, const size_t* outElts,
                               uint32_t* status, int maxWorkgroups, bool scatter, FlatScatterVParams* pp,
                               uint64_t* items) {
  FlatScatterVParams& p = *pp;
  const nexrResult_t res = flatCountedPrelude(n, inputs, outputs, counts, residence, esz, inElts, outElts, status,
                                              maxWorkgroups, (size_t)n, pp);
  if (res != nexrSuccess) return res;
  const size_t* own = scatter ? outElts : inElts;  // the capacities of the buffers that hold one piece
  *items = 0;
  if (residence == nexrScalarDevice) {
    for (int d = 0; d < n; d++) *items += ((uint64_t)own[d] * esz + 2047) / 2048;
    p.ext = counts;
  } else {
    uint64_t total = 0;
    if (!nexr_exchange_v::piecesFit(n, counts, inElts, outElts, scatter, &total)) return nexrInvalidArgument;
    for (int d = 0; d < n; d++) *items += (counts[d] * esz + 2047) / 2048;
    memcpy(p.counts, counts, (size_t)n * 8);
  }
  p.eszShift = eszShift(esz);
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatReduceScatterv(int nRanks, const void* const* inputs, void* const* outputs,
                                             const uint64_t* counts, int residence, int datatype, int devRedOp,
                                             uint64_t redOpArg, int userFirst, const size_t* inElts,
                                             const size_t* outElts, uint32_t* status, int maxWorkgroups,
                                             nexrStream_t stream) {
  nexrResult_t res = flatOpCheck(nRanks, datatype, devRedOp, redOpArg);
  if (res != nexrSuccess) return res;
  const size_t esz = typeSize(datatype);
  FlatScatterVParams p;
  memset((void*)&p, 0, sizeof(p));
  uint64_t items = 0;
  res = flatScatterVCheck(nRanks, inputs, outputs, counts, residence, esz, inElts, outElts, status, maxWorkgroups,
                          true, &p, &items);
  if (res != nexrSuccess) return res;
  for (int r = 0; r < nRanks; r++)
    if (((uintptr_t)inputs[r] | (uintptr_t)outputs[r]) & (esz - 1)) return nexrInvalidArgument;
  if (residence == nexrScalarHostImmediate && items == 0) return nexrSuccess;
  const FlatSemantics m = flatSemantics(nRanks, datatype, devRedOp, userFirst);
  p.redArg = redOpArg;
  p.userFirst = userFirst ? 1 : 0;
  p.nFold = m.nFold;
  p.shift = m.shift;
  p.preOp = m.preOp;
  p.postOp = m.postOp;
  unsigned grid = 0;
  res = flatCountedGrid(0, items, maxWorkgroups, &grid);
  if (res != nexrSuccess) return res;
  NEXR_HIP(launch_flat_scatter_v(m.dt, m.op, p, grid, (hipStream_t)stream));
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrFlatAllGatherv(int nRanks, const void* const* inputs, void* const* outputs,
                                         const uint64_t* counts, int residence, size_t esz, const size_t* inElts,
                                         const size_t* outElts, uint32_t* status, int maxWorkgroups,
                                         nexrStream_t stream) {
  if (!flatRanksOk(nRanks) || !eszOk(esz)) return nexrInvalidArgument;
  FlatScatterVParams p;
  memset((void*)&p, 0, sizeof(p));
  uint64_t items = 0;
  nexrResult_t res = flatScatterVCheck(nRanks, inputs, outputs, counts, residence, esz, inElts, outElts, status,
                                       maxWorkgroups, false, &p, &items);
  if (res != nexrSuccess) return res;
  if (residence == nexrScalarHostImmediate && items == 0) return nexrSuccess;
  unsigned grid = 0;
  res = flatCountedGrid(0, items, maxWorkgroups, &grid);
  if (res != nexrSuccess) return res;
  NEXR_HIP(launch_flat_gather_v(p, grid, (hipStream_t)stream));
  return nexrSuccess;
}

// ---- nexrFlatGroup, nexrFlatGroupPlan: several flat collectives as group launches -----------------------------
// The plan (no device call): every work through its single entry's checks, then the walk of include/nexr.h: one
// open launch per key, a conflict with a work of any open launch closes them all. Launches are queued in the
// order they were opened, at a cut and at the end alike, so a launch's number is its place in `launches`.
namespace {
struct GroupRange {
  uintptr_t beg, end;
};
struct GroupWork {  // a checked work with nElts > 0
  int index;        // in works[]
  int coll, key;
  int dt, op;       // the dispatch, after the semantics
  int root, isMin;
  int nFold, shift, preOp, postOp;
  uint64_t regionBytes, redArg, items;
  std::vector<GroupRange> rd, wr;
};
struct GroupLaunch {
  int key;
  std::vector<int> members;  // indices into the GroupWork list, in call order
  int maxOut = 0;            // copies: the longest destination list
  uint64_t nParts = 0, items = 0, tableBytes = 0;
  unsigned grid = 0;
  int fills = 0;
};
constexpr int kGroupCopyKey = -1;

bool groupHit(const std::vector<GroupRange>& a, const std::vector<GroupRange>& b) {
  for (const GroupRange& x : a)
    for (const GroupRange& y : b)
      if (x.beg < y.end && y.beg < x.end) return true;
  return false;
}
bool groupConflict(const GroupWork& a, const GroupWork& b) {
  return groupHit(a.wr, b.rd) || groupHit(a.wr, b.wr) || groupHit(b.wr, a.rd);
}

// A reduction work through its single entry's checks.
FlatCall groupWorkCheck(int nRanks, const nexrFlatGroupWork& w, int userFirst) {
  switch (w.coll) {
    case NEXR_FLAT_GROUP_ALL_REDUCE:
      return flatAllReduceCheck(nRanks, w.inputs, w.outputs, w.nElts, w.datatype, w.devRedOp, w.redOpArg, userFirst,
                                w.parts, w.nParts);
    case NEXR_FLAT_GROUP_REDUCE_SCATTER:
      return flatReduceScatterCheck(nRanks, w.inputs, w.outputs, w.nElts, w.datatype, w.devRedOp, w.redOpArg,
                                    userFirst);
    case NEXR_FLAT_GROUP_REDUCE:
      if (!w.outputs || w.root < 0 || w.root >= nRanks) break;
      return flatReduceCheck(nRanks, w.inputs, w.outputs[w.root], w.root, w.nElts, w.datatype, w.devRedOp, w.redOpArg,
                             userFirst);
  }
  return FlatCall();
}

nexrResult_t groupPlan(int nRanks, const nexrFlatGroupWork* works, int nWorks, int userFirst, int maxWorkgroups,
                       int* launchOf, nexrFlatGroupInfo* info, std::vector<GroupWork>* gwp,
                       std::vector<GroupLaunch>* lp) {
  std::vector<GroupWork>& gw = *gwp;
  std::vector<GroupLaunch>& launches = *lp;
  if (!works || nWorks < 0 || maxWorkgroups < 0 || !flatRanksOk(nRanks)) return nexrInvalidArgument;
  std::vector<int> placed((size_t)nWorks, -1);  // work -> its GroupWork
  for (int i = 0; i < nWorks; i++) {
    const nexrFlatGroupWork& w = works[i];
    GroupWork g;
    g.index = i;
    g.coll = w.coll;
    g.root = 0;
    g.isMin = 0;
    g.dt = g.op = 0;
    g.nFold = g.shift = g.preOp = g.postOp = 0;
    g.redArg = w.redOpArg;
    if (w.coll == NEXR_FLAT_GROUP_COPY) {
      if (!w.inputs || !w.inputs[0] || !w.outputs) return nexrInvalidArgument;
      if (w.nOutputs < 1 || w.nOutputs > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
      for (int r = 0; r < w.nOutputs; r++)
        if (!w.outputs[r]) return nexrInvalidArgument;
      g.key = kGroupCopyKey;
      g.regionBytes = w.nElts;
      g.items = ((uint64_t)w.nElts + 2047) / 2048;
      if (w.nElts) {
        const uintptr_t src = (uintptr_t)w.inputs[0];
        g.rd.push_back({src, src + w.nElts});
        for (int r = 0; r < w.nOutputs; r++)
          if ((uintptr_t)w.outputs[r] != src) g.wr.push_back({(uintptr_t)w.outputs[r], (uintptr_t)w.outputs[r] + w.nElts});
      }
    } else {
      const FlatCall c = groupWorkCheck(nRanks, w, userFirst);
      if (c.res != nexrSuccess) return c.res;
      const FlatParams& p = c.p;
      const bool minMax = w.devRedOp == nexrDevMinMax;
      g.isMin = minMax && (w.redOpArg & 1) == 0;
      g.key = w.datatype << 8 | w.devRedOp << 1 | (minMax ? (int)(w.redOpArg & 1) : 0);
      g.dt = c.dt;
      g.op = c.op;
      g.root = p.root;
      g.nFold = p.nFold;
      g.shift = p.shift;
      g.preOp = p.preOp;
      g.postOp = p.postOp;
      g.regionBytes = p.regionBytes;
      const int nRegions = w.coll == NEXR_FLAT_GROUP_REDUCE_SCATTER ? nRanks : 1;
      g.items = (p.regionBytes + 2047) / 2048 * (uint64_t)nRegions;
      const uint64_t inBytes = p.regionBytes * (uint64_t)nRegions;
      for (int r = 0; r < nRanks && w.nElts; r++) {
        g.rd.push_back({(uintptr_t)w.inputs[r], (uintptr_t)w.inputs[r] + inBytes});
        if (w.coll != NEXR_FLAT_GROUP_REDUCE || r == w.root)
          g.wr.push_back({(uintptr_t)w.outputs[r], (uintptr_t)w.outputs[r] + p.regionBytes});
      }
    }
    if (w.nElts == 0 || g.wr.empty()) continue;  // nothing to do: no launch, launchOf -1
    placed[i] = (int)gw.size();
    gw.push_back(std::move(g));
  }

  std::vector<int> open;         // open launches, in the order they were opened
  int cuts = 0;
  std::vector<int> launchOfGw(gw.size(), -1);
  for (size_t k = 0; k < gw.size(); k++) {
    bool cut = false;
    for (size_t o = 0; o < open.size() && !cut; o++)
      for (int m : launches[open[o]].members)
        if (groupConflict(gw[m], gw[k])) {
          cut = true;
          break;
        }
    if (cut) {
      open.clear();
      cuts++;
    }
    int at = -1;
    for (int o : open)
      if (launches[o].key == gw[k].key) at = o;
    if (at < 0) {
      at = (int)launches.size();
      launches.emplace_back();
      launches[at].key = gw[k].key;
      open.push_back(at);
    }
    GroupLaunch& L = launches[at];
    L.members.push_back((int)k);
    L.items += gw[k].items;
    const nexrFlatGroupWork& w = works[gw[k].index];
    if (gw[k].key == kGroupCopyKey) L.maxOut = std::max(L.maxOut, w.nOutputs);
    else if (gw[k].coll == NEXR_FLAT_GROUP_ALL_REDUCE) L.nParts += (uint64_t)w.nParts;
    launchOfGw[k] = at;
  }

  nexrFlatGroupInfo inf;
  memset(&inf, 0, sizeof(inf));
  inf.works = (int)gw.size();
  inf.launches = (int)launches.size();
  inf.cuts = cuts;
  for (GroupLaunch& L : launches) {
    const uint64_t W = L.members.size();
    L.tableBytes = L.key == kGroupCopyKey
                       ? W * (kFlatGroupCopyRecBytes + 8ull * (uint64_t)L.maxOut)
                       : W * (kFlatGroupRecBytes + 16ull * (uint64_t)nRanks) + L.nParts * sizeof(nexrFlatPart);
    if (L.tableBytes > 0xffffffffull) return nexrInvalidArgument;  // the pool's offset is 32 bits
    L.fills = L.tableBytes <= (uint64_t)kFlatGroupInlineBytes
                  ? 0
                  : (int)((L.tableBytes / 8 + kFlatGroupFillWords - 1) / kFlatGroupFillWords);
    L.grid = waveGrid(L.items, gridCap(kBlock), 0, (uint64_t)maxWorkgroups);
    inf.fillLaunches += L.fills;
    inf.tableBytes += L.tableBytes;
    inf.workgroups += L.grid;
  }
  if (launchOf)
    for (int i = 0; i < nWorks; i++) launchOf[i] = placed[i] < 0 ? -1 : launchOfGw[placed[i]];
  if (info) *info = inf;
  return nexrSuccess;
}

// The table of one launch, as nexr_internal.h lays it out.
void groupTable(const GroupLaunch& L, const std::vector<GroupWork>& gw, const nexrFlatGroupWork* works, int nRanks,
                std::vector<uint64_t>* tp, uint32_t* poolAt) {
  std::vector<uint64_t>& t = *tp;
  t.assign(L.tableBytes / 8, 0);
  uint64_t items = 0;
  if (L.key == kGroupCopyKey) {
    const size_t stride = (kFlatGroupCopyRecBytes + 8u * (size_t)L.maxOut) / 8;
    for (size_t k = 0; k < L.members.size(); k++) {
      const GroupWork& g = gw[L.members[k]];
      const nexrFlatGroupWork& w = works[g.index];
      uint64_t* rec = t.data() + k * stride;
      items += g.items;
      rec[0] = items;
      rec[1] = g.regionBytes;
      rec[2] = (uint64_t)(uintptr_t)w.inputs[0];
      for (int r = 0; r < w.nOutputs; r++) rec[3 + r] = w.outputs[r] == w.inputs[0] ? 0 : (uint64_t)(uintptr_t)w.outputs[r];
    }
    *poolAt = 0;
    return;
  }
  const size_t stride = (kFlatGroupRecBytes + 16u * (size_t)nRanks) / 8;
  const size_t pool = L.members.size() * stride;
  *poolAt = (uint32_t)(pool * 8);
  uint32_t partsAt = 0;
  for (size_t k = 0; k < L.members.size(); k++) {
    const GroupWork& g = gw[L.members[k]];
    const nexrFlatGroupWork& w = works[g.index];
    uint64_t* rec = t.data() + k * stride;
    items += g.items;
    const uint32_t nParts = g.coll == NEXR_FLAT_GROUP_ALL_REDUCE ? (uint32_t)w.nParts : 0u;
    rec[0] = items;
    rec[1] = g.regionBytes;
    rec[2] = g.redArg;
    rec[3] = (uint64_t)(uint32_t)g.coll | (uint64_t)(uint32_t)g.root << 32;
    rec[4] = (uint64_t)nParts | (uint64_t)partsAt << 32;
    for (int r = 0; r < nRanks; r++) {
      rec[5 + r] = (uint64_t)(uintptr_t)w.inputs[r];
      if (g.coll != NEXR_FLAT_GROUP_REDUCE || r == g.root) rec[5 + nRanks + r] = (uint64_t)(uintptr_t)w.outputs[r];
    }
    if (nParts) memcpy(t.data() + pool + (size_t)partsAt * 3, w.parts, (size_t)nParts * sizeof(nexrFlatPart));
    partsAt += nParts;
  }
}
static_assert(sizeof(nexrFlatPart) == 24, "the pool's entries are three words");
static_assert(kFlatGroupInlineBytes % 8 == 0, "a table of whole words rides inline or not at all");
}  // namespace

NEXR_API nexrResult_t nexrFlatGroupPlan(int nRanks, const nexrFlatGroupWork* works, int nWorks, int userFirst,
                                        int maxWorkgroups, int* launchOf, nexrFlatGroupInfo* info) {
  std::vector<GroupWork> gw;
  std::vector<GroupLaunch> launches;
  return groupPlan(nRanks, works, nWorks, userFirst, maxWorkgroups, launchOf, info, &gw, &launches);
}

NEXR_API nexrResult_t nexrFlatGroup(int nRanks, const nexrFlatGroupWork* works, int nWorks, int userFirst,
                                    int maxWorkgroups, int* launchOf, nexrFlatGroupInfo* info, nexrStream_t stream) {
  std::vector<GroupWork> gw;
  std::vector<GroupLaunch> launches;
  nexrResult_t res = groupPlan(nRanks, works, nWorks, userFirst, maxWorkgroups, launchOf, info, &gw, &launches);
  if (res != nexrSuccess) return res;
  hipStream_t s = (hipStream_t)stream;
  std::vector<uint64_t> table;
  // a launch with its table: inline up to kFlatGroupInlineBytes, else the L.fills launches of the plan ahead of it
  const auto withTable = [&](auto& p, auto&& launch) {
    return launchWithTable(table.data(), table.size(), (size_t)kFlatGroupInlineBytes / 8, p.inl, &p.ext, s, launch);
  };
  for (const GroupLaunch& L : launches) {
    uint32_t poolAt = 0;
    groupTable(L, gw, works, nRanks, &table, &poolAt);
    if (L.key == kGroupCopyKey) {
      FlatGroupCopyParams p;
      memset((void*)&p, 0, sizeof(p));
      p.nItems = L.items;
      p.nWorks = (int)L.members.size();
      p.maxOut = L.maxOut;
      res = withTable(p, [&] { return launch_flat_group_copy(p, L.grid, s); });
    } else {
      const GroupWork& g0 = gw[L.members[0]];
      FlatGroupParams p;
      memset((void*)&p, 0, sizeof(p));
      p.nItems = L.items;
      p.nWorks = (int)L.members.size();
      p.nRanks = nRanks;
      p.nFold = g0.nFold;
      p.shift = g0.shift;
      p.userFirst = userFirst ? 1 : 0;
      p.preOp = g0.preOp;
      p.postOp = g0.postOp;
      p.isMin = g0.isMin;
      p.poolAt = poolAt;
      res = withTable(p, [&] { return launch_flat_group(g0.dt, g0.op, p, L.grid, s); });
    }
    if (res != nexrSuccess) return res;
  }
  return nexrSuccess;
}

// ---- nexrFlatHost*: the flat entries over host memory -------------------------------------------------------
// The device entries' checks, then one helper for all six (flatHostRun). Every DISTINCT (address, length) among
// the call's buffers is classified once, as nexrReduceCopyHost classifies a buffer: the registration cache
// (regLookup, no HIP call), else the runtime's pointer query, trusted only when the whole buffer lies inside
// the pinned range it reports; a buffer that begins inside such a range and runs past its end is `cut`: never
// read in place, and copied only in pieces (hostCopyPieces). NEXR_HOST_ZERO_COPY=0 stages everything.
//   - Every buffer pinned: one launch over the device-mapped addresses, the grid capped at hostGrid().
//   - Otherwise a pageable input is copied into a device slot before the launch and a pageable output out of one
//     behind it; pinned buffers are still read and written in place. A host address always maps to the same
//     device address (pinned) or, as an input, to the same slot, so an input that appears twice is copied once.
//     Outputs that receive the same bytes (the all-reduces, the broadcast, the all-gather) share ONE staged
//     output, copied out once per distinct pageable output address. Every copy-in of a launch's bytes precedes
//     the launch and every copy-out follows it, and a lane stores a position only after it has read it from every
//     input, so the device entries' aliasing rules hold for host addresses as they stand.
//   - Calls whose inputs and outputs are one region (ring and tree all-reduce, reduce, broadcast) and that hold
//     more than one chunk (NEXR_FLAT_HOST_CHUNK_BYTES, 32 MiB, cut to a multiple of the 2048-byte piece) run as
//     a two-slot window pipeline on a pooled staging ring (stageFor): window w is copied in and launched on the
//     caller's stream while window w - 1 is copied out on the ring's stream. A staged window holds only its own
//     bytes, so its pointer is biased by -winBeg. The reduce-scatter and the all-gather stage whole: their
//     chunks are strided through the inputs and the outputs.
namespace {
std::atomic<uint64_t> gFhCalls{0}, gFhZeroCopy{0}, gFhStaged{0}, gFhRegHits{0}, gFhQueries{0}, gFhWindows{0};

struct FlatHostIo {
  int nIn = 0, nOut = 0;
  const void* in[NEXR_SYM_MAX_RANKS];  // host inputs, slot by slot
  void* out[NEXR_SYM_MAX_RANKS];       // host outputs, slot by slot; null: the slot has none
  size_t inBytes = 0, outBytes = 0;
  bool sharedOut = false;  // every output receives the same bytes: one staged output serves the pageable ones
  bool compact = false;    // the launch takes the distinct device outputs as a list, not slot by slot
  bool windowed = false;   // inputs and outputs are one region and the launch takes a byte window of it
  // a checked call's buffers: n inputs, nOutputs outputs
  void take(int n, const void* const* inputs, int nOutputs, void* const* outputs) {
    nIn = n;
    nOut = nOutputs;
    std::copy(inputs, inputs + n, in);
    std::copy(outputs, outputs + nOutputs, out);
  }
};
// (device inputs by slot, device outputs by slot or as the compact list, their number, winBeg, winEnd, the
// grid's cap or 0, stream)
using FlatHostLaunch = std::function<nexrResult_t(const char* const*, char* const*, int, uint64_t, uint64_t,
                                                  uint64_t, hipStream_t)>;

struct FlatHostBuf {
  uintptr_t host;
  size_t bytes;
  bool pin, cut;
  char* dev;    // pinned: the device address of the buffer
  int stageIn;  // pageable, used as an input: its slot among the staged inputs, else -1
  int stageOut; // pageable, used as an output: its slot among the staged outputs, else -1
};

// 32 MiB: with pageable buffers fewer windows were faster at every point measured (a 64 MiB all-reduce at 2 ranks:
// 6.18 ms in 4 MiB windows, 5.61 in 8, 5.21 in 16, 5.05 in 32, 5.02 whole; profiles/r19e_flat_host_chunk_sweep_64mib.json),
// so the chunk is what bounds the staging ring's memory, set where the loss to staging whole is 0.5 %.
size_t flatHostChunk() {
  static const long v = envLong("NEXR_FLAT_HOST_CHUNK_BYTES", 32l << 20);
  const size_t c = (size_t)(v > 2048 ? v : 2048);
  return c / 2048 * 2048;
}

int flatHostClassify(std::vector<FlatHostBuf>& bufs, const void* hp, size_t bytes, bool zeroCopy) {
  for (size_t i = 0; i < bufs.size(); i++)
    if (bufs[i].host == (uintptr_t)hp && bufs[i].bytes == bytes) return (int)i;
  FlatHostBuf b{(uintptr_t)hp, bytes, false, false, nullptr, -1, -1};
  void* dev = nullptr;
  if (!zeroCopy) {
    b.cut = true;  // what the runtime knows of the range is not asked: every copy goes in pieces
  } else if (regLookup(hp, bytes, &dev)) {
    b.pin = true;
    gFhRegHits.fetch_add(1, std::memory_order_relaxed);
  } else {
    gFhQueries.fetch_add(1, std::memory_order_relaxed);
    hipPointerAttribute_t a;
    b.pin = hipPointerGetAttributes(&a, hp) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer != nullptr;
    if (b.pin) {
      dev = a.devicePointer;
      uintptr_t beg = 0;
      size_t size = 0;
      if (hipPointerGetAttribute(&beg, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)hp) != hipSuccess ||
          hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)hp) != hipSuccess ||
          (uintptr_t)hp < beg || (uintptr_t)hp + bytes > beg + size) {
        b.pin = false;  // the device mapping ends before the buffer does
        b.cut = true;
      }
    }
    (void)hipGetLastError();  // pageable memory reports an error: not a failure of this call
  }
  b.dev = b.pin ? (char*)dev : nullptr;
  bufs.push_back(b);
  return (int)bufs.size() - 1;
}

nexrResult_t flatHostRun(const FlatHostIo& io, hipStream_t s, const FlatHostLaunch& launch) {
  static const long zeroCopy = envLong("NEXR_HOST_ZERO_COPY", 1);
  gFhCalls.fetch_add(1, std::memory_order_relaxed);
  std::vector<FlatHostBuf> bufs;
  int inIx[NEXR_SYM_MAX_RANKS], outIx[NEXR_SYM_MAX_RANKS];
  int nStageIn = 0, nStageOut = 0, nPinned = 0;
  for (int r = 0; r < io.nIn; r++) {
    inIx[r] = flatHostClassify(bufs, io.in[r], io.inBytes, zeroCopy != 0);
    FlatHostBuf& b = bufs[inIx[r]];
    if (!b.pin && b.stageIn < 0) b.stageIn = nStageIn++;
  }
  for (int r = 0; r < io.nOut; r++) {
    outIx[r] = -1;
    if (!io.out[r]) continue;
    outIx[r] = flatHostClassify(bufs, io.out[r], io.outBytes, zeroCopy != 0);
    FlatHostBuf& b = bufs[outIx[r]];
    if (!b.pin && b.stageOut < 0) b.stageOut = io.sharedOut ? 0 : nStageOut++;
    if (!b.pin && io.sharedOut) nStageOut = 1;
  }
  for (const FlatHostBuf& b : bufs) nPinned += b.pin ? 1 : 0;
  const char* devIn[NEXR_SYM_MAX_RANKS];
  char* devOut[NEXR_SYM_MAX_RANKS];
  // The launch's output list, a pageable output at its place behind outBase: slot by slot, or compact with
  // duplicates dropped. A staged window holds only its own bytes: the kernel addresses `pointer + region offset`.
  const auto listOutputs = [&](char* outBase, size_t outStride, uint64_t wb) {
    int m = 0;
    for (int r = 0; r < io.nOut; r++) {
      char* d = nullptr;
      if (outIx[r] >= 0) {
        const FlatHostBuf& b = bufs[outIx[r]];
        d = b.pin ? b.dev : outBase + outStride * (size_t)b.stageOut - wb;
      }
      if (!io.compact) {
        devOut[m++] = d;
      } else if (d && std::find(devOut, devOut + m, d) == devOut + m) {
        devOut[m++] = d;
      }
    }
    return m;
  };
  if (nStageIn + nStageOut == 0) {  // zero-copy: the kernel reads and writes the user buffers over the link
    gFhZeroCopy.fetch_add(1, std::memory_order_relaxed);
    gFhWindows.fetch_add(1, std::memory_order_relaxed);
    for (int r = 0; r < io.nIn; r++) devIn[r] = bufs[inIx[r]].dev;
    const int m = listOutputs(nullptr, 0, 0);  // every output is pinned
    const nexrResult_t res = launch(devIn, devOut, m, 0, io.windowed ? io.inBytes : 0, hostGrid(), s);
    if (res != nexrSuccess) return res;
    NEXR_HIP(hipStreamSynchronize(s));
    return nexrSuccess;
  }
  gFhStaged.fetch_add((uint64_t)(nStageIn + nStageOut), std::memory_order_relaxed);
  const size_t region = io.inBytes;
  const size_t chunk = io.windowed ? std::min(flatHostChunk(), (region + 2047) / 2048 * 2048) : 0;
  const size_t inStride = ((io.windowed ? chunk : io.inBytes) + 255) & ~(size_t)255;
  const size_t outStride = ((io.windowed ? chunk : io.outBytes) + 255) & ~(size_t)255;
  const size_t nWindows = io.windowed ? (region + chunk - 1) / chunk : 1;
  // A ring is two slots. A call of one window (every reduce-scatter and all-gather among them) uses the ring's
  // memory as ONE slot, so it asks for half its bytes a slot.
  const size_t slotNeed = inStride * (size_t)nStageIn + outStride * (size_t)nStageOut;
  StageLease lease;
  nexrResult_t res = stageFor(nWindows > 1 ? slotNeed : (slotNeed + 1) / 2, s, &lease);
  if (res != nexrSuccess) return res;
  HostStage* st = lease.st;
  gFhWindows.fetch_add(nWindows, std::memory_order_relaxed);
  for (size_t w = 0; w < nWindows; w++) {
    const int slot = (int)(w & 1);
    const uint64_t wb = io.windowed ? (uint64_t)w * chunk : 0;
    const uint64_t we = io.windowed ? std::min<uint64_t>(wb + chunk, region) : 0;
    const size_t inLen = io.windowed ? (size_t)(we - wb) : io.inBytes;
    const size_t outLen = io.windowed ? (size_t)(we - wb) : io.outBytes;
    char* inBase = st->buf + (nWindows > 1 ? (size_t)slot * st->slotBytes : 0);
    char* outBase = inBase + inStride * (size_t)nStageIn;
    if (w >= 2) NEXR_HIP(hipStreamWaitEvent(s, st->outDone[slot], 0));  // slot drained by window w - 2's copies out
    for (const FlatHostBuf& b : bufs) {
      if (b.stageIn < 0) continue;
      char* d = inBase + inStride * (size_t)b.stageIn;
      if (b.cut)
        NEXR_HIP(hostCopyPieces(d, (char*)b.host + wb, inLen, true, s));
      else
        NEXR_HIP(hipMemcpyAsync(d, (const char*)b.host + wb, inLen, hipMemcpyHostToDevice, s));
    }
    for (int r = 0; r < io.nIn; r++) {
      const FlatHostBuf& b = bufs[inIx[r]];
      devIn[r] = b.pin ? b.dev : inBase + inStride * (size_t)b.stageIn - wb;
    }
    const int m = listOutputs(outBase, outStride, wb);
    res = launch(devIn, devOut, m, wb, we, nPinned > 0 ? hostGrid() : 0, s);
    if (res != nexrSuccess) return res;
    if (nStageOut == 0) continue;
    NEXR_HIP(hipEventRecord(st->kernelDone[slot], s));
    NEXR_HIP(hipStreamWaitEvent(st->out, st->kernelDone[slot], 0));
    for (const FlatHostBuf& b : bufs) {
      if (b.stageOut < 0) continue;
      char* d = outBase + outStride * (size_t)b.stageOut;
      if (b.cut)
        NEXR_HIP(hostCopyPieces(d, (char*)b.host + wb, outLen, false, st->out));
      else
        NEXR_HIP(hipMemcpyAsync((char*)b.host + wb, d, outLen, hipMemcpyDeviceToHost, st->out));
    }
    NEXR_HIP(hipEventRecord(st->outDone[slot], st->out));
  }
  NEXR_HIP(hipStreamSynchronize(st->out));
  NEXR_HIP(hipStreamSynchronize(s));
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatHostAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, const nexrFlatPart* parts, int nParts,
                                            nexrStream_t stream) {
  FlatCall c = flatAllReduceCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst, parts,
                                  nParts);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  FlatParams& p = c.p;
  FlatHostIo io;
  io.take(nRanks, inputs, nRanks, outputs);
  io.inBytes = io.outBytes = (size_t)p.regionBytes;
  io.sharedOut = io.compact = io.windowed = true;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int nOut, uint64_t wb, uint64_t we, uint64_t cap,
                         hipStream_t s) {
                       for (int r = 0; r < nRanks; r++) {
                         p.in[r] = in[r];
                         p.out[r] = r < nOut ? out[r] : nullptr;
                       }
                       p.nOut = nOut;
                       p.winBeg = wb;
                       p.winEnd = we;
                       return flatLaunch(c, nullptr, 0, cap, s);
                     });
}

NEXR_API nexrResult_t nexrFlatHostReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                                size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                                int userFirst, nexrStream_t stream) {
  FlatCall c = flatReduceScatterCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  FlatParams& p = c.p;
  FlatHostIo io;
  io.take(nRanks, inputs, nRanks, outputs);
  io.outBytes = (size_t)p.regionBytes;
  io.inBytes = io.outBytes * (size_t)nRanks;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int, uint64_t, uint64_t, uint64_t cap,
                         hipStream_t s) {
                       for (int r = 0; r < nRanks; r++) {
                         p.in[r] = in[r];
                         p.out[r] = out[r];
                       }
                       return flatLaunch(c, nullptr, 0, cap, s);  // staged whole: the window stays the region
                     });
}

NEXR_API nexrResult_t nexrFlatHostReduce(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                                         int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                         nexrStream_t stream) {
  FlatCall c = flatReduceCheck(nRanks, inputs, output, root, nElts, datatype, devRedOp, redOpArg, userFirst);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  FlatParams& p = c.p;
  FlatHostIo io;
  io.take(nRanks, inputs, 1, &output);
  io.inBytes = io.outBytes = (size_t)p.regionBytes;
  io.windowed = true;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int, uint64_t wb, uint64_t we, uint64_t cap,
                         hipStream_t s) {
                       for (int r = 0; r < nRanks; r++) p.in[r] = in[r];
                       p.out[root] = out[0];
                       p.winBeg = wb;
                       p.winEnd = we;
                       return flatLaunch(c, nullptr, 0, cap, s);
                     });
}

NEXR_API nexrResult_t nexrFlatHostTreeAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                                size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                                int userFirst, const nexrFlatTreeLinks* const* trees, int nTrees,
                                                const nexrFlatTreePart* parts, int nParts, nexrStream_t stream) {
  FlatTreeCall c = flatTreeCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst, trees,
                                 nTrees, parts, nParts);
  if (c.res != nexrSuccess || nElts == 0) return c.res;
  FlatTreeParams& p = c.p;
  FlatHostIo io;
  io.take(nRanks, inputs, nRanks, outputs);
  io.inBytes = io.outBytes = (size_t)p.nBytes;
  io.sharedOut = io.compact = io.windowed = true;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int nOut, uint64_t wb, uint64_t we, uint64_t cap,
                         hipStream_t s) {
                       for (int r = 0; r < nRanks; r++) {
                         p.in[r] = in[r];
                         p.out[r] = r < nOut ? out[r] : nullptr;
                       }
                       p.nOut = nOut;
                       p.winBeg = wb;
                       p.winEnd = we;
                       return flatTreeLaunch(c, nullptr, 0, cap, s);
                     });
}

NEXR_API nexrResult_t nexrFlatHostBroadcast(int nRanks, const void* input, void* const* outputs, size_t nBytes,
                                            nexrStream_t stream) {
  if (!flatRanksOk(nRanks)) return nexrInvalidArgument;
  FlatHostIo io;
  bool any = false;
  if (!takeBroadcastOutputs(nRanks, input, outputs, io.out, &any)) return nexrInvalidArgument;
  if (nBytes == 0 || !any) return nexrSuccess;
  io.nIn = 1;
  io.nOut = nRanks;
  io.in[0] = input;
  io.inBytes = io.outBytes = nBytes;
  io.sharedOut = io.compact = io.windowed = true;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int nOut, uint64_t wb, uint64_t we, uint64_t cap,
                         hipStream_t s) {
                       FlatBcastParams p;
                       memset((void*)&p, 0, sizeof(p));
                       for (int r = 0; r < nOut; r++) p.out[r] = out[r];
                       p.in = in[0];
                       p.nBytes = nBytes;
                       p.winBeg = wb;
                       p.winEnd = we;
                       p.nRanks = nOut;
                       NEXR_HIP(launch_flat_bcast(p, flatGrid(we - wb, 1, cap), s));
                       return nexrSuccess;
                     });
}

NEXR_API nexrResult_t nexrFlatHostAllGather(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nBytes, nexrStream_t stream) {
  if (!flatRanksOk(nRanks)) return nexrInvalidArgument;
  if (nBytes > (size_t)-1 / (size_t)nRanks) return nexrInvalidArgument;  // an output's nRanks * nBytes bytes
  FlatHostIo io;
  if (!takeBuffers(nRanks, inputs, outputs, 0, &io)) return nexrInvalidArgument;
  if (nBytes == 0) return nexrSuccess;
  io.nIn = io.nOut = nRanks;
  io.inBytes = nBytes;
  io.outBytes = nBytes * (size_t)nRanks;
  io.sharedOut = true;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int, uint64_t, uint64_t, uint64_t cap,
                         hipStream_t s) {
                       SymAgParams p;
                       memset(&p, 0, sizeof(p));
                       std::copy(in, in + nRanks, p.in);
                       std::copy(out, out + nRanks, p.out);
                       // Pageable outputs all name the one staged output, which the kernel therefore
                       // stores once per pageable rank (the same bytes, in device memory: up to n times
                       // the device writes, none over the link). A staged buffer never lies inside another.
                       p.inPlace = symInPlace(p, nRanks, nBytes);
                       p.nBytes = nBytes;
                       p.nRanks = nRanks;
                       NEXR_HIP(launch_sym_all_gather(p, symChunkGrid(nBytes, 1, nRanks, cap), s));
                       return nexrSuccess;
                     });
}

NEXR_API nexrResult_t nexrGetFlatHostStats(nexrFlatHostStats* stats, int reset) {
  if (stats == nullptr) return nexrInvalidArgument;
  auto take = [&](std::atomic<uint64_t>& a) { return reset ? a.exchange(0) : a.load(); };
  stats->calls = take(gFhCalls);
  stats->zeroCopyCalls = take(gFhZeroCopy);
  stats->stagedBuffers = take(gFhStaged);
  stats->registeredHits = take(gFhRegHits);
  stats->pointerQueries = take(gFhQueries);
  stats->windows = take(gFhWindows);
  return nexrSuccess;
}

// ---- nexrSymLLAllReduce, nexrSymLLReduceScatter, nexrSymLLAllGather -----------------------------------------
// Two things make a launch finish: its grid of nRanks * nBlocks teams is resident as a whole (the occupancy
// check below), and every poll of its kernel is bounded (nexr_sym.hip). There is no dry run: a round needs
// nothing from a later launch.
NEXR_API nexrResult_t nexrSymLLWindowBytes(int nRanks, int maxBlocks, size_t* bytes) {
  if (!bytes || !flatRanksOk(nRanks) || maxBlocks < 1 || maxBlocks > NEXR_SYM_LL_MAX_BLOCKS)
    return nexrInvalidArgument;
  *bytes = (size_t)NEXR_SYM_LL_HEADER_BYTES + (size_t)maxBlocks * 2u * (size_t)nRanks * NEXR_SYM_LL_ROUND_PACKS * 16u;
  return nexrSuccess;
}

namespace {
// Workgroups of a symmetric LL kernel the current device keeps resident, as simpleGroupResident: the
// occupancy query's answer, capped at 4 per CU, less one (the query over-reports by one for 256-thread
// workgroups of kernels with many scalar registers; a surplus team would queue behind teams that poll it).
// Test hook: NEXR_TEST_SYM_LL_RESIDENT=k makes the next calls take k as that number (read per call).
nexrResult_t symLLResident(int coll, int dt, int64_t* resident) {
  static ResidentSlot cache[3][nexrNumTypes];
  return residentWorkgroups(
      ResidentLookup{"NEXR_TEST_SYM_LL_RESIDENT", &cache[coll][dt], sym_ll_blocks_per_cu, coll, dt, 4, true}, resident);
}

// The host side of the three calls. coll: 0 all-reduce (count elements per buffer), 1 reduce-scatter (count
// elements per chunk), 2 all-gather (count bytes, esz 1).
nexrResult_t symLL(int coll, int nRanks, const void* const* inputs, void* const* outputs, size_t count, int datatype,
                   void* const* windows, size_t windowBytes, int nBlocks, uint32_t* status, uint32_t timeoutUs,
                   nexrStream_t stream) {
  if (!inputs || !outputs || !windows) return nexrInvalidArgument;
  if (!flatRanksOk(nRanks) || nBlocks < 0 || nBlocks > NEXR_SYM_LL_MAX_BLOCKS) return nexrInvalidArgument;
  const int B = nBlocks ? nBlocks : 1;
  const uint64_t esz = coll == 2 ? 1 : typeSize(datatype);
  SymLLParams p;
  memset(&p, 0, sizeof(p));
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || !outputs[r] || !windows[r]) return nexrInvalidArgument;
    if (((uintptr_t)inputs[r] | (uintptr_t)outputs[r]) & (esz - 1)) return nexrInvalidArgument;
    if ((uintptr_t)windows[r] & 15) return nexrInvalidArgument;
    p.in[r] = (const char*)inputs[r];
    p.out[r] = (char*)outputs[r];
    p.win[r] = (char*)windows[r];
  }
  size_t need = 0;
  if (nexrSymLLWindowBytes(nRanks, B, &need) != nexrSuccess || windowBytes < need) return nexrInvalidArgument;
  // the reference's int nElts: a buffer (for the reduce-scatter the whole input) stays below 2^31 bytes
  const uint64_t limit = (1ull << 31) / esz / (coll == 1 ? (uint64_t)nRanks : 1u);
  if ((uint64_t)count >= limit) return nexrInvalidArgument;
  if (count == 0) return nexrSuccess;
  int64_t resident = 0;
  const nexrResult_t rr = symLLResident(coll, coll == 2 ? nexrFloat32 : datatype, &resident);
  if (rr != nexrSuccess) return rr;
  if ((int64_t)nRanks * B > resident) return nexrInvalidUsage;
  p.nBytes = (uint64_t)count * esz;
  p.status = status;
  p.timeoutTicks = pollTicks(timeoutUs);
  p.nRanks = nRanks;
  p.nBlocks = B;
  p.firstWins = semantics() == nexrSemanticsShipped;  // SKIP_COMP: every add returns its first operand
  NEXR_HIP(launch_sym_ll(coll, datatype, p, (hipStream_t)stream));
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrSymLLAllReduce(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                         int datatype, int devRedOp, uint64_t redOpArg, void* const* windows,
                                         size_t windowBytes, int nBlocks, uint32_t* status, uint32_t timeoutUs,
                                         nexrStream_t stream) {
  (void)redOpArg;
  if (datatype != nexrFloat32 && datatype != nexrFloat16 && datatype != nexrBfloat16) return nexrInvalidArgument;
  if (devRedOp != nexrDevSum) return nexrInvalidArgument;
  return symLL(0, nRanks, inputs, outputs, nElts, datatype, windows, windowBytes, nBlocks, status, timeoutUs, stream);
}

NEXR_API nexrResult_t nexrSymLLReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                             size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                             void* const* windows, size_t windowBytes, int nBlocks,
                                             uint32_t* status, uint32_t timeoutUs, nexrStream_t stream) {
  (void)redOpArg;
  if (datatype != nexrFloat32 && datatype != nexrFloat16 && datatype != nexrBfloat16) return nexrInvalidArgument;
  if (devRedOp != nexrDevSum) return nexrInvalidArgument;
  return symLL(1, nRanks, inputs, outputs, nElts, datatype, windows, windowBytes, nBlocks, status, timeoutUs, stream);
}

NEXR_API nexrResult_t nexrSymLLAllGather(int nRanks, const void* const* inputs, void* const* outputs, size_t nBytes,
                                         void* const* windows, size_t windowBytes, int nBlocks, uint32_t* status,
                                         uint32_t timeoutUs, nexrStream_t stream) {
  return symLL(2, nRanks, inputs, outputs, nBytes, nexrFloat32, windows, windowBytes, nBlocks, status, timeoutUs,
               stream);
}
