// steps_plan.cpp — the pure half of the step-list planner (nex-nccl_amd/csrc/nexr_steps_plan.h) driven without
// HIP: the launch cuts and the dry run over hand-made step lists, for a run under the host sanitizers
// (tests/test_native_sanitizers.py). Prints "steps_plan failures=N".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../nex-nccl_amd/csrc/nexr_steps_plan.h"

using namespace nexr;

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    failures++;
    printf("FAILED: %s\n", what);
  }
}

constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
char gInput[NEXR_LL_GROUP_MAX_MEMBERS][1024], gOutput[NEXR_LL_GROUP_MAX_MEMBERS][1024];
char gFifo[NEXR_LL_GROUP_MAX_MEMBERS * MP][16];  // only their addresses are used: a FIFO per connection

nexrLLStep step(int srcBuf, int64_t srcIx, int dstBuf, int64_t dstIx, uint32_t nElts, bool recv = false,
                bool send = false, uint8_t direct = 0) {
  nexrLLStep s;
  memset(&s, 0, sizeof(s));
  s.srcBuf = (int8_t)srcBuf, s.srcIx = srcIx, s.dstBuf = (int8_t)dstBuf, s.dstIx = dstIx, s.nElts = nElts;
  s.recv = recv, s.send = send, s.pad[0] = direct;
  return s;
}

// A group of members with their step lists; conn(m) wires what the case needs.
template <typename Params>
struct Group {
  std::vector<Params> cur;
  std::vector<std::vector<nexrLLStep>> lists;
  explicit Group(int n) : cur((size_t)n), lists((size_t)n) {
    for (int m = 0; m < n; m++) {
      memset((void*)&cur[(size_t)m], 0, sizeof(Params));
      cur[(size_t)m].input = gInput[m];
      cur[(size_t)m].output = gOutput[m];
      cur[(size_t)m].nSlots = 8;
    }
  }
  // member `from` sends on its next send connection to member `to`'s next receive connection
  void link(int from, int to, int fifo, uint64_t sent = 0, uint64_t read = 0) {
    Params& S = cur[(size_t)from];
    Params& R = cur[(size_t)to];
    S.sendFifo[S.nSend] = gFifo[fifo], S.sendStep[S.nSend++] = sent;
    R.recvFifo[R.nRecv] = gFifo[fifo], R.recvStep[R.nRecv++] = read;
  }
  void sendOnly(int from, int fifo, uint64_t sent) {
    Params& S = cur[(size_t)from];
    S.sendFifo[S.nSend] = gFifo[fifo], S.sendStep[S.nSend++] = sent;
  }
  void recvOnly(int to, int fifo, uint64_t read) {
    Params& R = cur[(size_t)to];
    R.recvFifo[R.nRecv] = gFifo[fifo], R.recvStep[R.nRecv++] = read;
  }
  // the plan: the refusal, or the launch count in *launches (the table in `table`)
  std::vector<Params> table;
  nexrResult_t plan(size_t* launches, uint64_t adv = 1, const nexrLLFlagRule* rule = nullptr) {
    std::vector<const nexrLLStep*> ptrs;
    std::vector<int> counts;
    for (auto& l : lists) ptrs.push_back(l.data()), counts.push_back((int)l.size());
    return planStepsGroup((int)cur.size(), cur.data(), ptrs.data(), counts.data(), 4, adv, 8, rule, &table, launches);
  }
  size_t count(uint64_t adv = 1, const nexrLLFlagRule* rule = nullptr) {
    size_t n = 0;
    return plan(&n, adv, rule) == nexrSuccess ? n : (size_t)-1;
  }
};

const nexrLLStep kSame = step(0, 0, 1, 0, 64);  // reads input[0, 64), writes output[0, 64)
const nexrLLStep kBack = step(1, 0, 0, 0, 64);  // reads output[0, 64), writes input[0, 64)
const nexrLLStep kSend = step(0, 0, -1, 0, 64, false, true);
const nexrLLStep kRecv = step(-1, 0, 1, 0, 64, true, false);

template <typename Params>
void cutCases(const char* form, uint64_t adv) {
  printf("cuts: %s\n", form);
  {
    Group<Params> g(1);
    g.lists[0].assign(96, kSame);
    expect(g.count(adv) == 1, "96 steps are one launch");
    expect(g.table[0].nSteps == 96, "... of 96 steps");
  }
  {
    Group<Params> g(1);
    g.lists[0].assign(97, kSame);
    expect(g.count(adv) == 2, "97 steps are two launches");
    expect(g.table[0].nSteps == 96 && g.table[1].nSteps == 1, "... of 96 and 1");
  }
  {
    Group<Params> g(2);
    g.lists[0].assign(100, kSame);
    g.lists[1].assign(3, kSame);
    expect(g.count(adv) == 2, "unequal members: two launches");
    expect(g.table[1].nSteps == 3 && g.table[3].nSteps == 0, "... the short member's steps in the first");
  }
  {
    Group<Params> g(1);
    g.lists[0] = {kBack, step(0, 0, 1, 1, 64)};
    expect(g.count(adv) == 2, "a write of a read range at another position cuts");
  }
  {
    Group<Params> g(1);
    g.lists[0] = {kBack, step(0, 0, 1, 0, 64)};
    expect(g.count(adv) == 1, "the same range at the same position does not");
  }
  {
    Group<Params> g(2);
    g.lists[0] = {kSame, kSame};
    g.lists[1] = {kBack, step(0, 0, 1, 1, 64)};
    expect(g.count(adv) == 2, "a conflict on one member cuts every member");
    expect(g.table[0].nSteps == 1 && g.table[2].nSteps == 1, "... at the same step index");
  }
  {  // the counters of the second launch stand behind the first launch's steps
    Group<Params> g(1);
    g.sendOnly(0, 0, 8 * adv);
    g.lists[0].assign(97, kSend);
    expect(g.count(adv) == 2, "97 sends, one-ended");
    expect(g.table[1].sendStep[0] == (8 + 96) * adv, "the second launch starts 96 sends on");
  }
}

void cleaningCases() {
  printf("cleaning steps\n");
  const nexrLLFlagRule rule{0x100, 0x78};
  const nexrLLStep copy = kSame;
  struct Case {
    uint64_t first;
    const char* steps;
    size_t want;
    uint32_t lastMask;  // cleanLast of the first launch
  } cases[] = {{0x76, "sss", 1, 1}, {0x77, "sss", 2, 1}, {0x77, "ssc", 2, 1}, {0x76, "scscs", 1, 1},
               {0x77, "scscs", 2, 1}, {0x7f, "sss", 2, 1}, {0x78, "ssss", 4, 1}, {0x70, "ssss", 1, 0}};
  for (const Case& c : cases) {
    Group<LLStepsParams> g(1);
    g.sendOnly(0, 0, c.first);
    for (const char* p = c.steps; *p; p++) g.lists[0].push_back(*p == 's' ? kSend : copy);
    expect(g.count(1, &rule) == c.want, c.steps);
    expect(g.table[0].cleanLast == c.lastMask, "cleanLast of the first launch");
    if (c.lastMask) expect((g.table[0].cleanStep[0] & 0x78) == 0x78, "cleanStep is the cleaning counter");
    Group<LLStepsParams> none(1);
    none.sendOnly(0, 0, c.first);
    none.lists[0] = g.lists[0];
    expect(none.count(1, nullptr) == 1, "no rule, no cleaning cut");
  }
  {  // two send connections at different counters: each cleans at its own
    Group<LLStepsParams> g(1);
    g.sendOnly(0, 0, 0x77);
    g.sendOnly(0, 1, 0x10);
    g.lists[0].assign(3, kSend);
    expect(g.count(1, &rule) == 2, "two connections: 0x78 on the first cuts");
    expect(g.table[0].cleanLast == 1 && g.table[1].cleanLast == 1, "only connection 0 cleans");
    expect(g.table[0].cleanStep[0] == 0x78 && g.table[1].cleanStep[0] == 0x79, "at 0x78 and 0x79");
  }
}

void directCases() {
  printf("direct receive\n");
  for (int ix = 0; ix < 2; ix++)
    for (int permit = 0; permit < 2; permit++)
      for (int direct = 0; direct < 2; direct++) {
        Group<SimpleDirectParams> g(1);
        g.recvOnly(0, 0, 0);
        g.cur[0].recvDirect = direct;
        g.cur[0].stepPerSlice = 2;
        g.lists[0] = {step(0, ix, 1, 1, 64),
                      step(-1, 0, 0, ix, 64, true, false, permit ? NEXR_SIMPLE_DIRECT_RECV : 0)};
        const size_t want = (ix == 0 && permit && direct) ? 2 : 1;
        expect(g.count(2) == want, "a direct source that conflicts cuts, and only then");
      }
}

// n members in a ring, member m sending to m + 1: the all-reduce's 2 (n - 1) steps, the first a send, the last
// a receive, the others receive and send.
void ringCases() {
  printf("rings\n");
  for (int n : {2, 8}) {
    Group<LLStepsParams> g(n);
    for (int m = 0; m < n; m++) g.link(m, (m + 1) % n, m);
    for (int m = 0; m < n; m++) {
      g.lists[(size_t)m].push_back(kSend);
      for (int k = 0; k < 2 * (n - 1) - 1; k++) g.lists[(size_t)m].push_back(step(0, 0, -1, 0, 64, true, true));
      g.lists[(size_t)m].push_back(kRecv);
    }
    size_t launches = 0;
    expect(g.plan(&launches) == nexrSuccess && launches == 1, "a ring finishes in one launch");
  }
  {  // the receiver waits for a step no member sends
    Group<LLStepsParams> g(2);
    g.link(0, 1, 0);
    g.lists[0] = {kSend};
    g.lists[1] = {kRecv, kRecv};
    size_t launches = 0;
    expect(g.plan(&launches) == nexrInvalidUsage, "a receive nobody sends is refused");
  }
  {  // both receive first
    Group<LLStepsParams> g(2);
    g.link(0, 1, 0);
    g.link(1, 0, 1);
    g.lists[0] = {kRecv, kSend};
    g.lists[1] = {kRecv, kSend};
    size_t launches = 0;
    expect(g.plan(&launches) == nexrInvalidUsage, "two members that wait for each other are refused");
  }
  {  // the read counter ahead of the sent counter
    Group<LLStepsParams> g(2);
    g.link(0, 1, 0, /*sent=*/0, /*read=*/3);
    g.lists[0] = {kSend};
    g.lists[1] = {kRecv};
    size_t launches = 0;
    expect(g.plan(&launches) == nexrInvalidUsage, "more read than sent is refused");
  }
  {  // credits: nine sends fit eight slots and one receive, ten do not; in slices of two steps, five and six
    for (uint64_t adv : {1, 2}) {
      const int fit = adv == 1 ? 9 : 5;
      for (int extra = 0; extra < 2; extra++) {
        Group<SimpleStepsParams> g(2);
        g.link(0, 1, 0);
        g.lists[0].assign((size_t)(fit + extra), kSend);
        g.lists[1] = {kRecv};
        size_t launches = 0;
        expect(g.plan(&launches, adv) == (extra ? nexrInvalidUsage : nexrSuccess), "the credit window");
      }
    }
  }
  {  // a step a later launch sends: the cut puts the send behind the receive that needs it
    Group<LLStepsParams> g(2);
    g.link(0, 1, 0);
    g.lists[0] = {kBack, step(0, 0, 1, 1, 64), kSend};  // cut before its second step: the send is in launch 2
    g.lists[1] = {kSame, kRecv};                        // the receive is step index 1: launch 2 as well
    size_t launches = 0;
    expect(g.plan(&launches) == nexrSuccess && launches == 2, "both in the second launch: fine");
    Group<LLStepsParams> h(2);
    h.link(0, 1, 0);
    h.lists[0] = {kBack, step(0, 0, 1, 1, 64), kSend};
    h.lists[1] = {kRecv};                               // launch 1 would wait for launch 2's send
    expect(h.plan(&launches) == nexrInvalidUsage, "a launch that waits for a later one is refused");
  }
  {  // the most members, three peers each way: member m sends to m + 1, m + 2, m + 3
    const int n = NEXR_LL_GROUP_MAX_MEMBERS;
    Group<LLStepsParams> g(n);
    for (int d = 1; d <= MP; d++)
      for (int m = 0; m < n; m++) g.link(m, (m + d) % n, (d - 1) * n + m);
    for (int m = 0; m < n; m++) g.lists[(size_t)m] = {kSend, kSend, kRecv, kRecv, kSend, kRecv};
    size_t launches = 0;
    expect(g.plan(&launches) == nexrSuccess && launches == 1, "32 members with three peers each finish");
    expect(g.cur[(size_t)n - 1].sendStep[MP - 1] == 3 && g.cur[0].recvStep[MP - 1] == 3, "counters behind the call");
  }
}
}  // namespace

int main() {
  cutCases<LLStepsParams>("LL / LL128", 1);
  cutCases<SimpleStepsParams>("SIMPLE", 2);
  cutCases<SimpleDirectParams>("SIMPLE direct", 2);
  cleaningCases();
  directCases();
  ringCases();
  printf("steps_plan failures=%d\n", failures);
  return failures ? 1 : 0;
}
