// nexr_steps_plan.h — the pure half of the step-list planner (nexr_steps_api.cpp submits what it returns): where a
// list of LL, LL128 or SIMPLE steps is cut into launches, and the dry run that refuses a group whose launch could
// not finish by itself. It works on the parameter blocks of nexr_internal.h, calls nothing from HIP and nothing
// with state, and compiles with a plain host compiler (tests/native/steps_plan.cpp runs it under sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nexr_internal.h"

namespace nexr {

// The steps run as if one at a time: a launch's workgroups walk its steps independently, which is
// only the same when no step touches user bytes that an earlier step of the launch wrote (or, for a
// write, read) at another element position. The same range at the same position is handled by the
// same lanes in both steps, in order.
struct UserRange {
  uintptr_t beg, end;  // end == 0: none
  bool write;
};
inline bool rangesConflict(const std::vector<UserRange>& seen, const UserRange& r) {
  for (const UserRange& q : seen) {
    if (!r.write && !q.write) continue;
    if (r.beg < q.end && q.beg < r.end && !(r.beg == q.beg && r.end == q.end)) return true;
  }
  return false;
}
inline UserRange userRange(const void* buf, int64_t ix, uint32_t nElts, size_t esz, bool write) {
  const uintptr_t beg = (uintptr_t)buf + (uintptr_t)ix * esz;
  return UserRange{beg, beg + (uintptr_t)nElts * esz, write};
}

// The user bytes a step reads and writes (srcBuf / dstBuf: 0 input, 1 output, -1 none).
struct StepRanges {
  UserRange rd, wr;
};
inline StepRanges stepRanges(const nexrLLStep& s, const void* input, const void* output, size_t esz) {
  StepRanges r{UserRange{0, 0, false}, UserRange{0, 0, true}};
  if (s.nElts && s.srcBuf >= 0) r.rd = userRange(s.srcBuf == 0 ? input : output, s.srcIx, s.nElts, esz, false);
  if (s.nElts && s.dstBuf >= 0) r.wr = userRange(s.dstBuf == 0 ? input : output, s.dstIx, s.nElts, esz, true);
  return r;
}

// incSend's cleanup (prims_ll.h:85-93): a send step whose counter has every bit of the mask set cleans
// its slot, per send connection. Bit j of the result: send connection j cleans at these counters.
inline uint32_t cleaningSends(const nexrLLFlagRule& rule, const uint64_t* sendCounters, int nSend) {
  uint32_t cleans = 0;
  for (int j = 0; j < nSend; j++)
    if (((uint32_t)sendCounters[j] & rule.cleanMask) == rule.cleanMask) cleans |= 1u << j;
  return cleans;
}

// What only one kind of table entry has. LLStepsParams carries the cleaning of its launch's last step: the
// launch ends at a cleaning step and its kernel cleans after its last step (nexr_ll.hip), so the step loop
// itself carries nothing for it. cleans == 0: the next launch starts with none.
inline void setCleaning(LLStepsParams& P, uint32_t cleans, const uint64_t* sendCounters) {
  P.cleanLast = cleans;
  for (int j = 0; j < NEXR_LL_STEPS_MAX_PEERS; j++)
    if (cleans & (1u << j)) P.cleanStep[j] = sendCounters[j];
}
inline void setCleaning(SimpleStepsParams&, uint32_t, const uint64_t*) {}  // SIMPLE has no flags to clean
// A SIMPLE direct receive reads the member's output at dstIx: a further user range the record reads.
inline UserRange directRead(const LLStepsParams&, const nexrLLStep&, size_t) { return UserRange{0, 0, false}; }
inline UserRange directRead(const SimpleStepsParams&, const nexrLLStep&, size_t) { return UserRange{0, 0, false}; }
inline UserRange directRead(const SimpleDirectParams& P, const nexrLLStep& s, size_t esz) {
  if (s.nElts && s.recv && (s.pad[0] & NEXR_SIMPLE_DIRECT_RECV) && P.recvDirect)
    return userRange(P.output, s.dstIx, s.nElts, esz, false);
  return UserRange{0, 0, false};
}

// The launch cuts. cur: the members' parameter blocks as they stand at the call's counters with no steps yet.
// A cut applies to every member at the same step index: before a step that would be a member's 97th of the
// launch or that conflicts with user bytes the member touched earlier in it (rangesConflict), and behind a
// step that cleans on any member under `rule` (nullptr: no cleaning steps; the kernel cleans behind a
// member's last step). emit(blocks) takes each complete launch, one block per member; the next launch starts
// at the counters behind it: a recv / send step advances a connection's counters by `adv` (1, or SIMPLE's
// stepPerSlice). The first result of emit that is not nexrSuccess ends the walk and is returned.
template <typename Params, typename Emit>
nexrResult_t cutLaunches(int nMembers, Params* cur, const nexrLLStep* const* steps, const int* nSteps, size_t esz,
                         uint64_t adv, const nexrLLFlagRule* rule, Emit emit) {
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  std::vector<std::vector<UserRange>> seen((size_t)nMembers);
  int maxSteps = 0;
  for (int m = 0; m < nMembers; m++) maxSteps = std::max(maxSteps, nSteps[m]);
  int inLaunch = 0;  // step indices in the current launch
  auto cut = [&]() -> nexrResult_t {
    const nexrResult_t r = emit((const Params*)cur);
    if (r != nexrSuccess) return r;
    for (int m = 0; m < nMembers; m++) {
      Params& P = cur[m];
      for (int k = 0; k < P.nSteps; k++) {
        const nexrLLStep& s = P.step[k];
        for (int i = 0; i < MP; i++) P.recvStep[i] += s.recv ? adv : 0, P.sendStep[i] += s.send ? adv : 0;
      }
      P.nSteps = 0;
      setCleaning(P, 0, nullptr);
      seen[(size_t)m].clear();
    }
    inLaunch = 0;
    return nexrSuccess;
  };
  for (int k = 0; k < maxSteps; k++) {
    bool before = inLaunch == kLLStepsMax, cleans = false;
    for (int m = 0; m < nMembers && !before; m++) {
      if (k >= nSteps[m]) continue;
      const StepRanges r = stepRanges(steps[m][k], cur[m].input, cur[m].output, esz);
      const UserRange rd2 = directRead(cur[m], steps[m][k], esz);
      before = (r.rd.end && rangesConflict(seen[(size_t)m], r.rd)) || (rd2.end && rangesConflict(seen[(size_t)m], rd2)) ||
               (r.wr.end && rangesConflict(seen[(size_t)m], r.wr));
    }
    if (before && inLaunch) {
      const nexrResult_t r = cut();
      if (r != nexrSuccess) return r;
    }
    for (int m = 0; m < nMembers; m++) {
      if (k >= nSteps[m]) continue;
      const nexrLLStep& s = steps[m][k];
      Params& P = cur[m];
      const StepRanges r = stepRanges(s, P.input, P.output, esz);
      const UserRange rd2 = directRead(P, s, esz);
      if (r.rd.end) seen[(size_t)m].push_back(r.rd);
      if (rd2.end) seen[(size_t)m].push_back(rd2);
      if (r.wr.end) seen[(size_t)m].push_back(r.wr);
      if (s.send && rule) {
        // the member's send counters at this step: those of the launch's start plus its send steps so far
        uint64_t at[MP];
        for (int j = 0; j < MP; j++) at[j] = P.sendStep[j];
        for (int q = 0; q < P.nSteps; q++)
          for (int j = 0; P.step[q].send && j < MP; j++) at[j] += adv;
        const uint32_t mask = cleaningSends(*rule, at, P.nSend);
        if (mask) {
          setCleaning(P, mask, at);
          cleans = true;
        }
      }
      P.step[P.nSteps++] = s;
    }
    inLaunch++;
    if (cleans) {
      const nexrResult_t r = cut();
      if (r != nexrSuccess) return r;
    }
  }
  return inLaunch ? cut() : nexrSuccess;
}

// The dry run: every launch must finish with what it and the launches before it produce, because the
// next one starts only behind it on the stream. Connections whose FIFO is some member's send FIFO and
// another's receive FIFO are internal: their data and credit counters are walked here; the others are
// taken as always ready (their peer runs elsewhere). table: nLaunches x nMembers blocks as cutLaunches
// emitted them. A slot is free again nSlots steps later. nexrInvalidUsage: some launch would wait for ever.
template <typename Params>
nexrResult_t dryRun(const Params* table, size_t nLaunches, int nMembers, uint64_t adv, uint64_t nSlots) {
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  struct Link {
    uint64_t sent, read;
  };
  if (nLaunches == 0) return nexrSuccess;
  std::vector<Link> links;
  std::vector<int> sendLink((size_t)nMembers * MP, -1), recvLink((size_t)nMembers * MP, -1);
  const Params* first = table;  // the first launch's blocks: the connections at the call's counters
  for (int m = 0; m < nMembers; m++)
    for (int j = 0; j < first[m].nSend; j++)
      for (int r = 0; r < nMembers && sendLink[(size_t)m * MP + j] < 0; r++)
        for (int i = 0; i < first[r].nRecv; i++)
          if ((const void*)first[r].recvFifo[i] == (const void*)first[m].sendFifo[j] &&
              recvLink[(size_t)r * MP + i] < 0) {
            if (first[m].sendStep[j] < first[r].recvStep[i]) return nexrInvalidUsage;  // more read than sent
            sendLink[(size_t)m * MP + j] = recvLink[(size_t)r * MP + i] = (int)links.size();
            links.push_back(Link{first[m].sendStep[j], first[r].recvStep[i]});
            break;
          }
  std::vector<int> pos((size_t)nMembers);
  for (size_t l = 0; l < nLaunches; l++) {
    const Params* L = table + l * (size_t)nMembers;
    std::fill(pos.begin(), pos.end(), 0);
    for (bool progress = true; progress;) {
      progress = false;
      for (int m = 0; m < nMembers; m++) {
        while (pos[(size_t)m] < L[m].nSteps) {
          const nexrLLStep& s = L[m].step[pos[(size_t)m]];
          bool ready = true;
          for (int i = 0; s.recv && i < L[m].nRecv; i++) {  // the line flags: the sender has written the step
            const int id = recvLink[(size_t)m * MP + i];
            if (id >= 0 && links[(size_t)id].sent < links[(size_t)id].read + adv) ready = false;
          }
          for (int j = 0; s.send && j < L[m].nSend; j++) {  // waitSend: the step nSlots back has been read
            const int id = sendLink[(size_t)m * MP + j];
            if (id >= 0 && links[(size_t)id].sent + adv > links[(size_t)id].read + nSlots) ready = false;
          }
          if (!ready) break;
          for (int i = 0; s.recv && i < L[m].nRecv; i++)
            if (recvLink[(size_t)m * MP + i] >= 0) links[(size_t)recvLink[(size_t)m * MP + i]].read += adv;
          for (int j = 0; s.send && j < L[m].nSend; j++)
            if (sendLink[(size_t)m * MP + j] >= 0) links[(size_t)sendLink[(size_t)m * MP + j]].sent += adv;
          pos[(size_t)m]++;
          progress = true;
        }
      }
    }
    for (int m = 0; m < nMembers; m++)
      if (pos[(size_t)m] < L[m].nSteps) return nexrInvalidUsage;  // this launch would wait for a later one
  }
  return nexrSuccess;
}

// The plan of a group call: the table (entry (launch l, member m) is that member's parameter block of launch l)
// and how many launches it holds, or the dry run's refusal. cur as cutLaunches takes it (and leaves it at the
// counters behind the last launch).
template <typename Params>
nexrResult_t planStepsGroup(int nMembers, Params* cur, const nexrLLStep* const* steps, const int* nSteps, size_t esz,
                            uint64_t adv, uint64_t nSlots, const nexrLLFlagRule* rule, std::vector<Params>* table,
                            size_t* nLaunches) {
  table->clear();
  cutLaunches(nMembers, cur, steps, nSteps, esz, adv, rule, [&](const Params* blocks) {
    table->insert(table->end(), blocks, blocks + nMembers);
    return nexrSuccess;
  });
  *nLaunches = table->size() / (size_t)nMembers;
  return dryRun(table->data(), *nLaunches, nMembers, adv, nSlots);
}

}  // namespace nexr
