// nexr_steps_api.cpp — the protocol step entries of the C ABI (include/nexr.h): the single LL / LL128 steps and
// the slot cleanup, the runs of LL steps of one Primitives, and the LL, LL128 and SIMPLE group launches with
// their workspace sizes. Host code only; the kernels live in nexr_ll.hip and nexr_simple.hip. The launch cuts
// and the dry run are nexr_steps_plan.h; what this file shares with nexr_api.cpp is declared in nexr_host.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "nexr_host.h"
#include "nexr_steps_plan.h"

using namespace nexr;

namespace {
constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;

// ---- the single steps: nexrReduceCopyLL, nexrReduceCopyLL128 -------------------------------------------------
// One body for both: Params is LLParams (32-bit flags) or LL128Params (64-bit flags), gridFor the workgroups
// that nBytes of data take, launch the kernel's launch function.
template <typename Params, typename Flag>
nexrResult_t llSingleStep(const void* src, int srcIsInput, int nRecv, const void* const* recvWire,
                          const Flag* recvFlags, void* dst, int nSend, void* const* sendWire, const Flag* sendFlags,
                          size_t nElts, int datatype, int devRedOp, uint64_t redOpArg, int postOp, uint32_t* status,
                          uint32_t timeoutUs, uint64_t (*gridFor)(uint64_t nBytes),
                          hipError_t (*launch)(int, const Params&, int, int, hipStream_t), nexrStream_t stream) {
  if (nRecv < 0 || nRecv > NEXR_MAX_SRCS || nSend < 0 || nSend > NEXR_MAX_DSTS) return nexrInvalidArgument;
  if (!src && nRecv == 0) return nexrInvalidArgument;   // LLGenericOp needs SRC or RECV
  if (!dst && nSend == 0) return nexrInvalidArgument;   // ... and DST or SEND
  if (!typeOpOk(datatype, devRedOp, redOpArg)) return nexrInvalidArgument;
  if ((nRecv && (!recvWire || !recvFlags)) || (nSend && (!sendWire || !sendFlags))) return nexrInvalidArgument;
  if (nElts == 0) return nexrSuccess;
  Params a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < nRecv; i++) {
    if (!recvWire[i] || ((uintptr_t)recvWire[i] & 15)) return nexrInvalidArgument;
    a.recv[i] = (const char*)recvWire[i];
    a.recvFlag[i] = recvFlags[i];
  }
  for (int i = 0; i < nSend; i++) {
    if (!sendWire[i] || ((uintptr_t)sendWire[i] & 15)) return nexrInvalidArgument;
    a.send[i] = (char*)sendWire[i];
    a.sendFlag[i] = sendFlags[i];
  }
  a.src = (const char*)src;
  a.dst = (char*)dst;
  a.nElts = nElts;
  a.redArg = redOpArg;
  a.status = status;
  a.timeoutTicks = pollTicks(timeoutUs);
  a.nRecv = nRecv;
  a.nSend = nSend;
  a.srcIsInput = srcIsInput ? 1 : 0;
  a.postOp = postOp ? 1 : 0;
  llSemantics(&datatype, &devRedOp, &a.srcIsInput, &a.postOp, &a.firstWins);
  uint64_t grid = gridFor(nElts * typeSize(datatype));
  if (grid > (1u << 20)) grid = 1u << 20;
  NEXR_HIP(launch(datatype, a, devRedOp, (int)grid, (hipStream_t)stream));
  return nexrSuccess;
}

// 8 data bytes per 16-byte line, a workgroup per tile of kLLTileLines lines.
uint64_t llGrid(uint64_t nBytes) { return ((nBytes + 7) / 8 + kLLTileLines - 1) / kLLTileLines; }
// 1920 data bytes per 2 KiB slice of 128 wire units, a workgroup per tile of kLL128TileUnits units.
uint64_t ll128Grid(uint64_t nBytes) {
  const uint64_t nUnits = (nBytes + kLL128SliceData - 1) / kLL128SliceData * 128;
  return (nUnits + kLL128TileUnits - 1) / kLL128TileUnits;
}
}  // namespace

extern "C" {

NEXR_API nexrResult_t nexrReduceCopyLL(const void* src, int srcIsInput, int nRecv, const void* const* recvLines,
                                       const uint32_t* recvFlags, void* dst, int nSend, void* const* sendLines,
                                       const uint32_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                       uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                       nexrStream_t stream) {
  return llSingleStep<LLParams, uint32_t>(src, srcIsInput, nRecv, recvLines, recvFlags, dst, nSend, sendLines,
                                          sendFlags, nElts, datatype, devRedOp, redOpArg, postOp, status, timeoutUs,
                                          llGrid, launch_ll, stream);
}

NEXR_API nexrResult_t nexrReduceCopyLL128(const void* src, int srcIsInput, int nRecv, const void* const* recvWire,
                                          const uint64_t* recvFlags, void* dst, int nSend, void* const* sendWire,
                                          const uint64_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                          uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                          nexrStream_t stream) {
  return llSingleStep<LL128Params, uint64_t>(src, srcIsInput, nRecv, recvWire, recvFlags, dst, nSend, sendWire,
                                             sendFlags, nElts, datatype, devRedOp, redOpArg, postOp, status,
                                             timeoutUs, ll128Grid, launch_ll128, stream);
}

NEXR_API nexrResult_t nexrLLCleanSlot(int nSend, void* const* sendLines, const uint32_t* sendFlags, size_t firstLine,
                                      size_t slotLines, nexrStream_t stream) {
  if (nSend < 0 || nSend > NEXR_MAX_DSTS) return nexrInvalidArgument;
  if (nSend && (!sendLines || !sendFlags)) return nexrInvalidArgument;
  LLCleanParams a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < nSend; i++) {
    if (!sendLines[i] || ((uintptr_t)sendLines[i] & 15)) return nexrInvalidArgument;
    a.send[i] = (char*)sendLines[i];
    a.flag[i] = sendFlags[i];
  }
  if (nSend == 0 || firstLine >= slotLines) return nexrSuccess;
  a.firstLine = firstLine;
  a.slotLines = slotLines;
  a.nSend = nSend;
  // One workgroup per line tile from the first one that holds a clean line (the kernel skips those before it).
  const uint64_t slotTiles = (slotLines + kLLTileLines - 1) / kLLTileLines;
  uint64_t grid = slotTiles - firstLine / kLLTileLines;
  if (grid > 1024) grid = 1024;
  NEXR_HIP(launch_ll_clean(a, (int)grid, (hipStream_t)stream));
  return nexrSuccess;
}

}  // extern "C"

// ---- what the step lists of every protocol share ---------------------------------------------------------------
namespace {
// A flag rule is valid for nSlots slots (include/nexr.h): flagMax 0 or a power of two, cleanMask != 0 and a
// multiple of nSlots (the reference's static_assert, prims_ll.h), and the cleaning period
// 2^(msb(cleanMask) + 1) within the flag period, so that every line is rewritten before its flag recurs.
bool llRuleValid(const nexrLLFlagRule& r, uint32_t nSlots) {
  if (r.flagMax & (r.flagMax - 1)) return false;
  if (r.cleanMask == 0 || nSlots == 0 || r.cleanMask % nSlots) return false;
  const uint64_t cleanPeriod = 2ull << (31 - __builtin_clz(r.cleanMask));
  const uint64_t flagPeriod = r.flagMax ? (uint64_t)r.flagMax : 1ull << 32;
  return cleanPeriod <= flagPeriod;
}
const nexrLLFlagRule kProductionRule{0u, 0x7ffffff8u};

// The connections of a nexrLLConnSet or nexrSimpleConnSet: the peer counts, slots that are whole multiples of
// slotUnit bytes, a slot count the kernels can keep as an int, and FIFO and head pointers that are set and
// aligned.
template <typename ConnSet>
bool connSetOk(const ConnSet& cs, uint64_t slotUnit) {
  if (cs.nRecv < 0 || cs.nRecv > MP || cs.nSend < 0 || cs.nSend > MP) return false;
  if (cs.slotBytes == 0 || cs.slotBytes % slotUnit || cs.nSlots == 0 || cs.nSlots > (uint32_t)INT_MAX) return false;
  for (int i = 0; i < cs.nRecv; i++)
    if (!cs.recvFifo[i] || ((uintptr_t)cs.recvFifo[i] & 15) || !cs.recvHead[i] || ((uintptr_t)cs.recvHead[i] & 7))
      return false;
  for (int i = 0; i < cs.nSend; i++)
    if (!cs.sendFifo[i] || ((uintptr_t)cs.sendFifo[i] & 15) || !cs.sendHead[i] || ((uintptr_t)cs.sendHead[i] & 7))
      return false;
  return true;
}

// The steps of one member against its connections. wireBytes bounds what a step carries: LL and LL128 bound a
// step that receives or sends by the slot's data bytes (boundEveryStep false), SIMPLE every non-empty step by
// the slice.
template <typename ConnSet>
bool stepListOk(const ConnSet& cs, const nexrLLStep* steps, int nSteps, size_t esz, uint64_t wireBytes,
                bool boundEveryStep) {
  if (nSteps < 0 || (nSteps > 0 && !steps)) return false;
  for (int k = 0; k < nSteps; k++) {
    const nexrLLStep& s = steps[k];
    if (s.srcBuf < -1 || s.srcBuf > 1 || s.dstBuf < -1 || s.dstBuf > 1) return false;
    if ((s.recv && cs.nRecv == 0) || (s.send && cs.nSend == 0)) return false;
    if ((s.srcBuf == 0 && !cs.input) || (s.srcBuf == 1 && !cs.output) || (s.dstBuf == 0 && !cs.input) ||
        (s.dstBuf == 1 && !cs.output))
      return false;
    if (s.srcIx < 0 || s.dstIx < 0) return false;
    if (s.nElts == 0) continue;
    if ((s.srcBuf < 0 && !s.recv) || (s.dstBuf < 0 && !s.send)) return false;
    if ((boundEveryStep || s.recv || s.send) && (uint64_t)s.nElts * esz > wireBytes) return false;
  }
  return true;
}

// The argument checks of a run of LL steps of one Primitives (nexrReduceCopyLLStepsRule, and every member
// of nexrReduceCopyLLStepsGroup): nothing here touches the device. rule == nullptr: LL128 steps (every
// member of nexrReduceCopyLL128StepsGroup), whose slots are whole 2 KiB slices of 1920 data bytes and whose
// 64-bit flags need no rule.
nexrResult_t llStepsValidate(const nexrLLConnSet* cs, const nexrLLStep* steps, int nSteps, int datatype, int devRedOp,
                             uint64_t redOpArg, const nexrLLFlagRule* rule) {
  if (!cs || !connSetOk(*cs, rule ? 16 : kLL128SliceBytes)) return nexrInvalidArgument;
  if (rule && !llRuleValid(*rule, cs->nSlots)) return nexrInvalidArgument;
  if (!typeOpOk(datatype, devRedOp, redOpArg)) return nexrInvalidArgument;
  // 8 data bytes per 16-byte line; LL128: 1920 per 2 KiB slice
  const uint64_t slotData = rule ? cs->slotBytes / 2 : cs->slotBytes / kLL128SliceBytes * kLL128SliceData;
  if (!stepListOk(*cs, steps, nSteps, typeSize(datatype), slotData, false)) return nexrInvalidArgument;
  return nexrSuccess;
}

// The fields every step-list parameter block takes from its connection set and the call (the block zeroed
// first); what only one form has (flagMask, tails, stepPerSlice, the direct fields) is set beside the call.
template <typename Params, typename ConnSet>
void fillConnFields(Params& P, const ConnSet& cs, uint64_t redOpArg, uint32_t* status, uint32_t timeoutUs,
                    int firstWins) {
  memset((void*)&P, 0, sizeof(P));
  P.input = (const char*)cs.input;
  P.output = (char*)cs.output;
  for (int i = 0; i < MP; i++) {
    P.recvFifo[i] = (const char*)cs.recvFifo[i];
    P.recvHead[i] = cs.recvHead[i];
    P.sendFifo[i] = (char*)cs.sendFifo[i];
    P.sendHead[i] = cs.sendHead[i];
    P.recvStep[i] = cs.recvStep[i];
    P.sendStep[i] = cs.sendStep[i];
  }
  P.slotBytes = cs.slotBytes;
  P.redArg = redOpArg;
  P.status = status;
  P.timeoutTicks = pollTicks(timeoutUs);
  P.nRecv = cs.nRecv;
  P.nSend = cs.nSend;
  P.nSlots = (int)cs.nSlots;
  P.firstWins = firstWins;
}

// One workgroup per tile of a full LL / LL128 slot (the same grid on both ends of every connection): a tile is
// kLLTileLines 16-byte lines, or kLL128TileUnits 16-byte wire units.
int workgroupsPerSlot(uint64_t slotBytes, uint64_t tileUnits) {
  const uint64_t slotTiles = (slotBytes / 16 + tileUnits - 1) / tileUnits;
  return (int)(slotTiles < 1 ? 1 : slotTiles > (uint64_t)kLLStepsMaxGrid ? kLLStepsMaxGrid : slotTiles);
}

// The workspace of a group call: a region of nMembers table entries for each of NEXR_LL_GROUP_LAUNCHES launches.
nexrResult_t groupWorkspaceBytes(int nMembers, size_t entryBytes, size_t* bytes) {
  if (!bytes || nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS) return nexrInvalidArgument;
  *bytes = (size_t)nMembers * entryBytes * NEXR_LL_GROUP_LAUNCHES;
  return nexrSuccess;
}
}  // namespace

extern "C" {

NEXR_API nexrResult_t nexrReduceCopyLLSteps(const nexrLLConnSet* cs, const nexrLLStep* steps, int nSteps,
                                            int datatype, int devRedOp, uint64_t redOpArg, uint32_t* status,
                                            uint32_t timeoutUs, nexrStream_t stream) {
  return nexrReduceCopyLLStepsRule(cs, steps, nSteps, datatype, devRedOp, redOpArg, nullptr, status, timeoutUs,
                                   stream);
}

// The one-member caller of the cutter: each launch's block goes to the kernel by value as soon as it is cut,
// with no table, no dry run and no workspace.
NEXR_API nexrResult_t nexrReduceCopyLLStepsRule(const nexrLLConnSet* cs, const nexrLLStep* steps, int nSteps,
                                                int datatype, int devRedOp, uint64_t redOpArg,
                                                const nexrLLFlagRule* rulePtr, uint32_t* status, uint32_t timeoutUs,
                                                nexrStream_t stream) {
  const nexrLLFlagRule rule = rulePtr ? *rulePtr : kProductionRule;  // NULL: the production rule
  const nexrResult_t valid = llStepsValidate(cs, steps, nSteps, datatype, devRedOp, redOpArg, &rule);
  if (valid != nexrSuccess) return valid;
  if (nSteps == 0) return nexrSuccess;
  const size_t esz = typeSize(datatype);
  int srcIsInput = 1, postOp = 1, firstWins = 0;
  llSemantics(&datatype, &devRedOp, &srcIsInput, &postOp, &firstWins);
  LLStepsParams P;
  fillConnFields(P, *cs, redOpArg, status, timeoutUs, firstWins);
  P.flagMask = rule.flagMax ? rule.flagMax - 1 : 0xffffffffu;
  const int grid = workgroupsPerSlot(cs->slotBytes, kLLTileLines);
  return cutLaunches(1, &P, &steps, &nSteps, esz, 1, &rule, [&](const LLStepsParams* block) -> nexrResult_t {
    NEXR_HIP(launch_ll_steps(datatype, *block, devRedOp, grid, (hipStream_t)stream));
    return nexrSuccess;
  });
}

}  // extern "C"

// ---- the group launches: the step lists of several Primitives in one launch ----------------------------------
// Three things make a group launch finish: its grid is resident as a whole (the occupancy
// check below), it needs nothing a later launch would produce (the dry run), and every poll of its
// kernel is bounded (nexr_ll.hip, nexr_simple.hip).
namespace {
// Workgroups of the LL or LL128 group kernel the current device keeps resident, looked up once per (device,
// datatype, op): the occupancy query's answer as it is.
// Test hook: NEXR_TEST_LL_GROUP_RESIDENT=k makes the next calls take k as that number, so that the
// rejection of a grid that does not fit (and the ring's fall-back) can be tested on a GPU that fits it.
ResidentLookup llGroupResident(bool ll128, int dt, int op) {
  static ResidentSlot cache[2][nexrNumTypes][nexrNumDevRedOps];  // [LL, LL128]: a kernel each
  return ResidentLookup{"NEXR_TEST_LL_GROUP_RESIDENT", &cache[ll128][dt][op],
                        ll128 ? ll128_group_blocks_per_cu : ll_group_blocks_per_cu, dt, op, 0, false};
}

// Workgroups of the SIMPLE group kernel the current device keeps resident, as llGroupResident. The
// hardware admits 256-thread workgroups by their scalar registers too, and for kernels that use more than
// 80 of them one fewer per CU than the occupancy query says; a surplus workgroup would queue until a
// resident one exits, which a poll may be waiting for. So one is taken off the query's answer, capped at 8.
// Test hook: NEXR_TEST_SIMPLE_GROUP_RESIDENT=k makes the next calls take k as that number.
// direct: the kernel variant of nexrReduceCopySimpleStepsGroupDirect (the one that is launched is queried).
ResidentLookup simpleGroupResident(bool direct, int dt, int op) {
  static ResidentSlot cache[2][nexrNumTypes][nexrNumDevRedOps];  // [FIFO-only, direct]
  return ResidentLookup{"NEXR_TEST_SIMPLE_GROUP_RESIDENT", &cache[direct][dt][op],
                        direct ? simple_group_direct_blocks_per_cu : simple_group_blocks_per_cu, dt, op, 8, true};
}

// The submit half of a group call, behind its argument checks: the plan (nexr_steps_plan.h: the launch cuts
// and the dry run), the workspace fit, the residency of nMembers * G workgroups, the one copy of the tables
// and the launches. cur: the members' parameter blocks at the call's counters with no steps yet.
template <typename Params>
nexrResult_t submitStepsGroup(int nMembers, std::vector<Params>& cur, const nexrLLStep* const* steps,
                              const int* nSteps, size_t esz, uint64_t adv, uint64_t nSlots,
                              const nexrLLFlagRule* rule, int G, const ResidentLookup& kernel,
                              hipError_t (*launch)(int, int, const Params*, int, int, hipStream_t), int datatype,
                              int devRedOp, void* workspace, size_t workspaceBytes, nexrStream_t stream) {
  std::vector<Params> table;
  size_t nLaunches = 0;
  const nexrResult_t plan = planStepsGroup(nMembers, cur.data(), steps, nSteps, esz, adv, nSlots, rule, &table,
                                           &nLaunches);
  if (plan != nexrSuccess) return plan;

  // One region of the workspace per launch: a table is never written while a queued launch may read it.
  if (workspaceBytes / sizeof(Params) / (size_t)nMembers < nLaunches) return nexrInvalidArgument;

  // Co-residency: all nMembers * G workgroups at once, or a poll could wait for a workgroup that has no CU.
  int64_t resident = 0;
  const nexrResult_t occ = residentWorkgroups(kernel, &resident);
  if (occ != nexrSuccess) return occ;
  if ((int64_t)nMembers * G > resident) return nexrInvalidUsage;

  // Pageable source: the runtime has staged it when the call returns, so `table` may go out of scope.
  NEXR_HIP(hipMemcpyAsync(workspace, table.data(), table.size() * sizeof(Params), hipMemcpyHostToDevice,
                          (hipStream_t)stream));
  for (size_t l = 0; l < nLaunches; l++)
    NEXR_HIP(launch(datatype, devRedOp, (const Params*)workspace + l * (size_t)nMembers, nMembers, G,
                    (hipStream_t)stream));
  return nexrSuccess;
}

// The host side of both LL group calls. rule == nullptr: LL128 steps (nexrReduceCopyLL128StepsGroup), which
// have no cleaning steps (so no cut behind one), slots counted in 2 KiB slices and a kernel (and so an
// occupancy) of their own; everything else is the same code.
nexrResult_t llStepsGroup(int nMembers, const nexrLLConnSet* conns, const nexrLLStep* const* steps, const int* nSteps,
                          int datatype, int devRedOp, uint64_t redOpArg, const nexrLLFlagRule* rule, uint32_t* status,
                          uint32_t timeoutUs, void* workspace, size_t workspaceBytes, nexrStream_t stream) {
  const bool ll128 = rule == nullptr;
  if (nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS || !conns || !steps || !nSteps) return nexrInvalidArgument;
  int maxSteps = 0;
  for (int m = 0; m < nMembers; m++) {
    const nexrResult_t valid = llStepsValidate(&conns[m], steps[m], nSteps[m], datatype, devRedOp, redOpArg, rule);
    if (valid != nexrSuccess) return valid;
    // one G (a workgroup per line tile of a slot) and one credit window serve the launch
    if (conns[m].slotBytes != conns[0].slotBytes || conns[m].nSlots != conns[0].nSlots) return nexrInvalidArgument;
    maxSteps = std::max(maxSteps, nSteps[m]);
  }
  if (maxSteps == 0) return nexrSuccess;
  if (!workspace || ((uintptr_t)workspace & 7)) return nexrInvalidArgument;
  const size_t esz = typeSize(datatype);
  int srcIsInput = 1, postOp = 1, firstWins = 0;
  llSemantics(&datatype, &devRedOp, &srcIsInput, &postOp, &firstWins);
  std::vector<LLStepsParams> cur((size_t)nMembers);
  for (int m = 0; m < nMembers; m++) {
    fillConnFields(cur[(size_t)m], conns[m], redOpArg, status, timeoutUs, firstWins);
    cur[(size_t)m].flagMask = rule && rule->flagMax ? rule->flagMax - 1 : 0xffffffffu;
  }
  const int G = workgroupsPerSlot(conns[0].slotBytes, ll128 ? kLL128TileUnits : kLLTileLines);
  return submitStepsGroup(nMembers, cur, steps, nSteps, esz, 1, conns[0].nSlots, rule, G,
                          llGroupResident(ll128, datatype, devRedOp), ll128 ? launch_ll128_group : launch_ll_group,
                          datatype, devRedOp, workspace, workspaceBytes, stream);
}

// What a nexrSimpleConnSet has beyond connSetOk: the tail words, and counters in whole slices.
bool simpleConnSetOk(const nexrSimpleConnSet& cs) {
  if (cs.stepPerSlice < 1 || cs.nSlots % cs.stepPerSlice) return false;
  for (int i = 0; i < cs.nRecv; i++)
    if (!cs.recvTail[i] || ((uintptr_t)cs.recvTail[i] & 7) || cs.recvStep[i] % cs.stepPerSlice) return false;
  for (int i = 0; i < cs.nSend; i++)
    if (!cs.sendTail[i] || ((uintptr_t)cs.sendTail[i] & 7) || cs.sendStep[i] % cs.stepPerSlice) return false;
  return true;
}

// The SIMPLE fields of a table entry, beside the common ones.
template <typename Params>
void fillSimple(Params& P, const nexrSimpleConnSet& cs, uint64_t redOpArg, uint32_t* status, uint32_t timeoutUs,
                int firstWins) {
  fillConnFields(P, cs, redOpArg, status, timeoutUs, firstWins);
  for (int i = 0; i < MP; i++) P.recvTail[i] = cs.recvTail[i], P.sendTail[i] = cs.sendTail[i];
  P.stepPerSlice = (int)cs.stepPerSlice;
}

// The host side of both SIMPLE group calls. direct == nullptr: nexrReduceCopySimpleStepsGroup, the FIFO-only
// kernels and their table entry; else one nexrSimpleDirectSet per member, the direct kernels and theirs.
nexrResult_t simpleStepsGroup(int nMembers, const nexrSimpleConnSet* conns, const nexrLLStep* const* steps,
                              const int* nSteps, int datatype, int devRedOp, uint64_t redOpArg,
                              int workgroupsPerMember, const nexrSimpleDirectSet* direct, uint32_t* status,
                              uint32_t timeoutUs, void* workspace, size_t workspaceBytes, nexrStream_t stream) {
  if (nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS || !conns || !steps || !nSteps) return nexrInvalidArgument;
  if (workgroupsPerMember < 0 || workgroupsPerMember > NEXR_SIMPLE_GROUP_MAX_GRID) return nexrInvalidArgument;
  if (!typeOpOk(datatype, devRedOp, redOpArg)) return nexrInvalidArgument;
  const size_t esz = typeSize(datatype);
  int maxSteps = 0;
  for (int m = 0; m < nMembers; m++) {
    const nexrSimpleConnSet& cs = conns[m];
    if (!connSetOk(cs, 16) || !simpleConnSetOk(cs)) return nexrInvalidArgument;
    // one G, one credit window and one slice size serve the launch
    if (cs.slotBytes != conns[0].slotBytes || cs.nSlots != conns[0].nSlots || cs.stepPerSlice != conns[0].stepPerSlice)
      return nexrInvalidArgument;
    if (!stepListOk(cs, steps[m], nSteps[m], esz, cs.slotBytes * cs.stepPerSlice, true)) return nexrInvalidArgument;
    maxSteps = std::max(maxSteps, nSteps[m]);
  }
  if (direct) {
    // Only one receive may be direct (prims_simple.h:262), and its source is the member's output.
    for (int m = 0; m < nMembers; m++) {
      bool any = false;
      for (int i = 0; i < MP; i++) any = any || direct[m].recvDirect[i] != 0;
      if (any && (conns[m].nRecv != 1 || !direct[m].recvDirect[0] || !conns[m].output)) return nexrInvalidArgument;
    }
    // A connection between two members is direct on both ends or on neither, into the receiver's output.
    for (int m = 0; m < nMembers; m++)
      for (int j = 0; j < conns[m].nSend; j++)
        for (int r = 0; r < nMembers; r++)
          for (int i = 0; i < conns[r].nRecv; i++) {
            if (conns[r].recvFifo[i] != conns[m].sendFifo[j]) continue;
            const void* sd = direct[m].sendDirect[j];
            if ((sd != nullptr) != (direct[r].recvDirect[i] != 0)) return nexrInvalidArgument;
            if (sd && sd != conns[r].output) return nexrInvalidArgument;
          }
  }
  if (maxSteps == 0) return nexrSuccess;
  if (!workspace || ((uintptr_t)workspace & 7)) return nexrInvalidArgument;
  const uint64_t sps = conns[0].stepPerSlice;
  int srcIsInput = 1, postOp = 1, firstWins = 0;
  llSemantics(&datatype, &devRedOp, &srcIsInput, &postOp, &firstWins);  // fork: the dispatch type; shipped: source 0
  // A workgroup per 4 KiB tile of a full slice unless the caller says how many.
  const uint64_t sliceTiles = (conns[0].slotBytes * sps + kSimpleTileBytes - 1) / kSimpleTileBytes;
  const int G = workgroupsPerMember ? workgroupsPerMember
                                    : (int)(sliceTiles > (uint64_t)kSimpleMaxGrid ? kSimpleMaxGrid : sliceTiles);
  if (direct) {
    std::vector<SimpleDirectParams> cur((size_t)nMembers);
    for (int m = 0; m < nMembers; m++) {
      SimpleDirectParams& P = cur[(size_t)m];
      fillSimple(P, conns[m], redOpArg, status, timeoutUs, firstWins);
      for (int j = 0; j < conns[m].nSend; j++) P.sendDirect[j] = (char*)direct[m].sendDirect[j];
      P.recvDirect = direct[m].recvDirect[0] ? 1 : 0;
    }
    return submitStepsGroup(nMembers, cur, steps, nSteps, esz, sps, conns[0].nSlots, nullptr, G,
                            simpleGroupResident(true, datatype, devRedOp), launch_simple_group_direct, datatype,
                            devRedOp, workspace, workspaceBytes, stream);
  }
  std::vector<SimpleStepsParams> cur((size_t)nMembers);
  for (int m = 0; m < nMembers; m++) fillSimple(cur[(size_t)m], conns[m], redOpArg, status, timeoutUs, firstWins);
  return submitStepsGroup(nMembers, cur, steps, nSteps, esz, sps, conns[0].nSlots, nullptr, G,
                          simpleGroupResident(false, datatype, devRedOp), launch_simple_group, datatype, devRedOp,
                          workspace, workspaceBytes, stream);
}
}  // namespace

extern "C" {

NEXR_API nexrResult_t nexrLLGroupWorkspaceBytes(int nMembers, size_t* bytes) {
  return groupWorkspaceBytes(nMembers, kLLGroupEntryBytes, bytes);
}

NEXR_API nexrResult_t nexrReduceCopyLLStepsGroup(int nMembers, const nexrLLConnSet* conns,
                                                 const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                 int devRedOp, uint64_t redOpArg, const nexrLLFlagRule* rulePtr,
                                                 uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                 size_t workspaceBytes, nexrStream_t stream) {
  const nexrLLFlagRule rule = rulePtr ? *rulePtr : kProductionRule;  // NULL: the production rule
  return llStepsGroup(nMembers, conns, steps, nSteps, datatype, devRedOp, redOpArg, &rule, status, timeoutUs,
                      workspace, workspaceBytes, stream);
}

NEXR_API nexrResult_t nexrReduceCopyLL128StepsGroup(int nMembers, const nexrLLConnSet* conns,
                                                    const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                    int devRedOp, uint64_t redOpArg, uint32_t* status,
                                                    uint32_t timeoutUs, void* workspace, size_t workspaceBytes,
                                                    nexrStream_t stream) {
  return llStepsGroup(nMembers, conns, steps, nSteps, datatype, devRedOp, redOpArg, nullptr, status, timeoutUs,
                      workspace, workspaceBytes, stream);
}

NEXR_API nexrResult_t nexrSimpleGroupWorkspaceBytes(int nMembers, size_t* bytes) {
  return groupWorkspaceBytes(nMembers, sizeof(SimpleStepsParams), bytes);
}

NEXR_API nexrResult_t nexrReduceCopySimpleStepsGroup(int nMembers, const nexrSimpleConnSet* conns,
                                                     const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                     int devRedOp, uint64_t redOpArg, int workgroupsPerMember,
                                                     uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                     size_t workspaceBytes, nexrStream_t stream) {
  return simpleStepsGroup(nMembers, conns, steps, nSteps, datatype, devRedOp, redOpArg, workgroupsPerMember, nullptr,
                          status, timeoutUs, workspace, workspaceBytes, stream);
}

NEXR_API nexrResult_t nexrSimpleGroupDirectWorkspaceBytes(int nMembers, size_t* bytes) {
  return groupWorkspaceBytes(nMembers, sizeof(SimpleDirectParams), bytes);
}

NEXR_API nexrResult_t nexrReduceCopySimpleStepsGroupDirect(int nMembers, const nexrSimpleConnSet* conns,
                                                           const nexrLLStep* const* steps, const int* nSteps,
                                                           int datatype, int devRedOp, uint64_t redOpArg,
                                                           int workgroupsPerMember, const nexrSimpleDirectSet* direct,
                                                           uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                           size_t workspaceBytes, nexrStream_t stream) {
  return simpleStepsGroup(nMembers, conns, steps, nSteps, datatype, devRedOp, redOpArg, workgroupsPerMember, direct,
                          status, timeoutUs, workspace, workspaceBytes, stream);
}

}  // extern "C"
