// nexr_api.cpp — the C ABI (include/nexr.h): argument validation, datatype/op dispatch, launch
// geometry, the host-staged variant and the op encoder. Host code only; the kernels live in
// nexr_kernels.hip (one object per datatype).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "nexr_internal.h"

namespace nexr {
namespace {

thread_local int tLastHipError = 0;

inline nexrResult_t hipFail(hipError_t e) {
  tLastHipError = (int)e;
  return nexrUnhandledCudaError;
}
#define NEXR_HIP(call)                          \
  do {                                          \
    hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hipFail(e_);   \
  } while (0)

// ---- host-path counters (nexrGetHostPathStats): where a nexrReduceCopyHost call spends its time
std::atomic<uint64_t> gHpCalls{0}, gHpZeroCopy{0}, gHpRegHits{0}, gHpQueries{0};
std::atomic<uint64_t> gHpClassifyNs{0}, gHpCopyNs{0}, gHpLaunchNs{0}, gHpWaitNs{0};
inline uint64_t nowNs() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}


size_t typeSize(int dt) {
  switch (dt) {
    case nexrInt8: case nexrUint8: case nexrFloat8e4m3: case nexrFloat8e5m2: return 1;
    case nexrFloat16: case nexrBfloat16: return 2;
    case nexrInt32: case nexrUint32: case nexrFloat32: return 4;
    case nexrInt64: case nexrUint64: case nexrFloat64: return 8;
  }
  return 0;
}
bool isInteger(int dt) { return dt >= nexrInt8 && dt <= nexrUint64; }
bool isSignedInt(int dt) { return dt == nexrInt8 || dt == nexrInt32 || dt == nexrInt64; }

long envLong(const char* name, long dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return strtol(v, nullptr, 0);
}

// Reduction semantics (include/nexr.h, nexrSetSemantics): process-wide, like an NCCL parameter; the
// initial value comes from NEXR_SEMANTICS the first time a call needs it.
std::atomic<int> gSemantics{-1};

int semantics() {
  int s = gSemantics.load(std::memory_order_relaxed);
  if (s >= 0) return s;
  const char* v = getenv("NEXR_SEMANTICS");
  int init = nexrSemanticsNccl;
  if (v && (!strcmp(v, "fork") || !strcmp(v, "1"))) init = nexrSemanticsFork;
  if (v && (!strcmp(v, "shipped") || !strcmp(v, "2"))) init = nexrSemanticsShipped;
  gSemantics.compare_exchange_strong(s, init);
  return gSemantics.load(std::memory_order_relaxed);
}

// The fork's kernel dispatch (equivalent_primary, generate.py:128-136): signed Min/Max run on the
// unsigned kernel, whose FuncMinMax never applies the sign xormask hostToDevRedOp encodes.
int forkDispatchType(int dt, int op) {
  if (op != nexrDevMinMax) return dt;
  switch (dt) {
    case nexrInt8: return nexrUint8;
    case nexrInt32: return nexrUint32;
    case nexrInt64: return nexrUint64;
  }
  return dt;
}

// The parts of a validated SIMPLE call the semantics can change. Shipped (SKIP_COMP): every reduce
// returns acc = src0, the pre-op and post-op return their input — a K = 1 copy with no arithmetic.
struct CallShape {
  int dt, op, nSrcs, nPreOp, postOp;
  const void* prePtr;
};
void applySemantics(CallShape& c) {
  const int s = semantics();
  if (s == nexrSemanticsFork) {
    c.dt = forkDispatchType(c.dt, c.op);
  } else if (s == nexrSemanticsShipped) {
    c.op = nexrDevSum;
    c.nSrcs = 1;
    c.nPreOp = 0;
    c.postOp = 0;
    c.prePtr = nullptr;
  }
}

// The kernel a (semantics-shaped) call runs: kernel_compiled (nexr_internal.h) names the compiled
// ones; every other call maps onto one of them with the same output bytes. A K = 1 copy becomes a
// byte copy (*nElts counted in bytes from then on); signed Sum / Prod / PreMulSum / SumPostDiv run the
// unsigned kernel; PreMulSum without pre-op sources and SumPostDiv without the divide run Sum.
int unsignedOf(int dt) {
  return dt == nexrInt8 ? nexrUint8 : dt == nexrInt32 ? nexrUint32 : dt == nexrInt64 ? nexrUint64 : dt;
}
void routeKernel(CallShape& c, size_t* nElts) {
  if (c.op == nexrDevPreMulSum && c.nPreOp == 0) c.op = nexrDevSum;
  if (c.op == nexrDevSumPostDiv && !c.postOp) c.op = nexrDevSum;
  if (c.nSrcs == 1 && c.op != nexrDevPreMulSum && c.op != nexrDevSumPostDiv) {
    *nElts *= typeSize(c.dt);
    c.dt = nexrUint8;
    c.op = nexrDevSum;
    return;
  }
  if (c.op != nexrDevMinMax) c.dt = unsignedOf(c.dt);
}

// The same for an LL / LL128 step (after validation): shipped → every reduce returns its first operand,
// the peer (prims_ll.h:288-294, prims_ll128.h:225-255), with no pre-op and no post-op.
void llSemantics(int* dt, int* op, int* srcIsInput, int* postOp, int* firstWins) {
  const int s = semantics();
  *firstWins = 0;
  if (s == nexrSemanticsFork) {
    *dt = forkDispatchType(*dt, *op);
  } else if (s == nexrSemanticsShipped) {
    *op = nexrDevSum;
    *srcIsInput = 0;
    *postOp = 0;
    *firstWins = 1;
  }
}

// Cache policy by the bytes a call streams (every src read once, every dst written once): plain below
// NEXR_NT_LOAD_MIN_BYTES (64 MiB: the data likely sits in L2/MALL and the consumer wants the output
// there too), non-temporal loads above it, non-temporal loads and stores above
// NEXR_NT_STORE_MIN_BYTES (512 MiB = 2x the Infinity Cache). NEXR_POLICY (0/1/3) overrides it for
// sweeps. The workgroup geometry follows the policy (unroll_for/block_for, nexr_internal.h).
// One exception (round 5): calls with few sources take nt stores as well from
// NEXR_NT_STORE_K2_MIN_BYTES (96 MiB streamed), for the (K, M) measured to gain at 96-510 MiB
// (tools/occupancy_ab.hip ntstore / ntstore2 / ntstore3 / c4pol / ntstore4): K = 1 with M = 1-4
// (1.1-4.8 %), K = 2 with M = 1-7 (2.2-6.3 %; M = 7, round 6: 0.7-2.4 %), K = 3 with M = 2-7 (3.1-5.6 %;
// M = 6-7, round 6: 0-5.0 %, never slower) (profiles/r05q_occupancy_ntstore.txt,
// r05zd_occupancy_ntstore2.txt, r05zg_occupancy_ntstore3.txt, r05zj_occupancy_ntstore3_m5.txt,
// r06w_occupancy_ntstore4.txt). Outside it nt stores were mixed (K = 3 M = 1, K = 1 M = 5, K = 2 M = 8
// and K = 3 M = 8: 1.3-4.8 % slower at 110-120 MiB, 2.3-4.7 % faster at 290-300) or lost (K = 1 M = 8:
// 2.9-5.9 %, K = 4 M = 2, K = 8). nDsts = 0: unknown (a batch), the general rule.
constexpr int kNtStoreMinM[4] = {0, 1, 1, 2}, kNtStoreMaxM[4] = {0, 4, 7, 7};
int pickPolicy(uint64_t streamBytes, int nSrcs = 0, int nDsts = 0) {
  static const long polOverride = envLong("NEXR_POLICY", -1);
  static const long ntLoadMin = envLong("NEXR_NT_LOAD_MIN_BYTES", 64l << 20);
  static const long ntStoreMin = envLong("NEXR_NT_STORE_MIN_BYTES", 512l << 20);
  static const long ntStoreK2Min = envLong("NEXR_NT_STORE_K2_MIN_BYTES", 96l << 20);
  if (polOverride >= 0) return polOverride == 0 ? 0 : (polOverride == 1 ? 1 : 3);
  const bool fewSrcs = nSrcs >= 1 && nSrcs <= 3 && nDsts >= kNtStoreMinM[nSrcs] && nDsts <= kNtStoreMaxM[nSrcs];
  if (fewSrcs && streamBytes >= (uint64_t)ntStoreK2Min) return 3;
  return streamBytes >= (uint64_t)ntStoreMin ? 3 : (streamBytes >= (uint64_t)ntLoadMin ? 1 : 0);
}

// Grid: one workgroup per kTripPacks-pack trip ("one-shot"), capped so that grid x block stays
// within HIP's 2^32 - 1 work-item limit (2^24 workgroups of 256 lanes, 2^22 of 1024); beyond the
// cap the kernel grid-strides. NEXR_GRID overrides the grid for sweeps.
uint64_t gridCap(int block) { return 0xffffffffull / (uint64_t)block; }

nexrResult_t pickGeometry(uint64_t workgroups, int pol, int block, Geometry* g) {
  static const long gridOverride = envLong("NEXR_GRID", 0);
  const uint64_t cap = gridCap(block);
  uint64_t need = workgroups < 1 ? 1 : workgroups;
  g->grid = (int)(need < cap ? need : cap);
  if (gridOverride > 0) g->grid = (int)gridOverride;
  g->pol = pol;
  return nexrSuccess;
}

hipError_t launchDt(int dt, const RCParams& p, int op, int nSrcs, const Geometry& g, hipStream_t s) {
  switch (dt) {
    case 0: return launch_dt0(p, op, nSrcs, g, s);
    case 1: return launch_dt1(p, op, nSrcs, g, s);
    case 2: return launch_dt2(p, op, nSrcs, g, s);
    case 3: return launch_dt3(p, op, nSrcs, g, s);
    case 4: return launch_dt4(p, op, nSrcs, g, s);
    case 5: return launch_dt5(p, op, nSrcs, g, s);
    case 6: return launch_dt6(p, op, nSrcs, g, s);
    case 7: return launch_dt7(p, op, nSrcs, g, s);
    case 8: return launch_dt8(p, op, nSrcs, g, s);
    case 9: return launch_dt9(p, op, nSrcs, g, s);
  }
  return hipErrorInvalidValue;
}

// Shared validation for every reduce-copy entry point (error convention: SURVEY §8(b)).
nexrResult_t validate(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts, size_t nElts,
                      int datatype, int op, uint64_t redOpArg, int nPreOpSrcs, const uint64_t* preOpArgs) {
  if (nSrcs < 1 || nSrcs > NEXR_MAX_SRCS) return nexrInvalidArgument;
  if (nDsts < 0 || nDsts > NEXR_MAX_DSTS) return nexrInvalidArgument;
  if (datatype < 0 || datatype >= nexrNumTypes) return nexrInvalidArgument;
  if (datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2) return nexrInvalidArgument;
  if (op < 0 || op >= nexrNumDevRedOps) return nexrInvalidArgument;
  // SumPostDiv kernels exist for integer types only (generate.py:108 required_cuda).
  if (op == nexrDevSumPostDiv && !isInteger(datatype)) return nexrInvalidArgument;
  if (op == nexrDevSumPostDiv && (redOpArg & 1) != 0) {
    // The signed quotient (taken by bit 0 of redOpArg, whatever the datatype's own signedness:
    // reduce_kernel.h:79-97) divides by the divisor truncated to T (:94): a divisor that
    // truncates to 0 would divide by zero. Only a 1-byte T can truncate a non-zero divisor to 0.
    uint32_t divisor = (uint32_t)(redOpArg >> 1);
    if (divisor == 0) divisor = 1;
    size_t sz = typeSize(datatype);
    if (sz == 1 && (int8_t)divisor == 0) return nexrInvalidArgument;
  }
  if (nPreOpSrcs < 0 || nPreOpSrcs > nSrcs) return nexrInvalidArgument;
  if (nPreOpSrcs > 0 && preOpArgs == nullptr) return nexrInvalidArgument;
  if (nElts == 0 || nDsts == 0) return nexrSuccess;
  if (srcs == nullptr || (nDsts > 0 && dsts == nullptr)) return nexrInvalidArgument;
  for (int s = 0; s < nSrcs; s++)
    if (srcs[s] == nullptr) return nexrInvalidArgument;
  for (int d = 0; d < nDsts; d++)
    if (dsts[d] == nullptr) return nexrInvalidArgument;
  return nexrSuccess;
}

// Split [0, nElts) into head edge / packed body / tail edge (RCParams comment). Pack i of the body
// is the 16 contiguous bytes at offset 16 i of every buffer, at that buffer's own alignment: when all
// pointers share a 16-B phase every access is aligned; otherwise the misaligned ones are unaligned
// 16-B loads / stores (one instruction per lane on gfx950, no element-by-element path). The head
// brings the first destination to a 128-B boundary when its offset is a whole number of elements, so
// that each wave's 1 KiB store instruction writes whole 128-B lines: misaligned stores cost more than
// misaligned loads (tools/misalign_rate.py).
constexpr uintptr_t kLineBytes = 128;
void planLayout(RCParams& p, int nSrcs, size_t esz) {
  const uintptr_t phase16 = (uintptr_t)p.src[0] & 15;
  bool common = (phase16 % esz) == 0;
  for (int s = 1; s < nSrcs && common; s++) common = (((uintptr_t)p.src[s]) & 15) == phase16;
  for (int d = 0; d < p.nDsts && common; d++) common = (((uintptr_t)p.dst[d]) & 15) == phase16;
  p.unaligned = common ? 0 : 1;
  uintptr_t phase = (uintptr_t)p.dst[0] & (kLineBytes - 1);
  if (phase % esz) phase = 0;
  uint64_t head = phase ? (kLineBytes - phase) / esz : 0;
  if (head > p.nElts) head = p.nElts;
  p.head = head;
  p.nPacks = (p.nElts - head) * esz / 16;
}

void fillParams(RCParams& p, int nSrcs, const void* const* srcs, int nDsts, void* const* dsts, size_t nElts,
                size_t esz, uint64_t redOpArg, int nPreOpSrcs, const uint64_t* preOpArgs, const void* prePtr,
                int postOp) {
  memset(&p, 0, sizeof(p));
  for (int s = 0; s < nSrcs; s++) p.src[s] = (const char*)srcs[s];
  for (int d = 0; d < nDsts; d++) p.dst[d] = (char*)dsts[d];
  for (int s = 0; s < nPreOpSrcs; s++) p.pre[s] = preOpArgs[s];
  p.prePtr = prePtr;
  p.redArg = redOpArg;
  p.nElts = nElts;
  p.nDsts = nDsts;
  p.nPreOp = nPreOpSrcs;
  p.postOp = postOp ? 1 : 0;
  planLayout(p, nSrcs, esz);
}

// One-shot workgroups of one reduce-copy: one per B lane work items, a work item being a U-pack
// group, with (U, B) = the kernel's geometry for (dt, K, policy).
uint64_t workgroupsFor(const RCParams& p, int nSrcs, int dt, int pol) {
  const uint64_t u = (uint64_t)unroll_for(dt, nSrcs, pol), b = (uint64_t)block_for(dt, nSrcs, pol);
  const uint64_t items = (p.nPacks + u - 1) / u;  // >= 1 workgroup (pickGeometry) covers the edges
  return (items + b - 1) / b;
}

hipError_t launchBatchDt(int dt, const BatchParams& b, int op, int nSrcs, int pol, int grid, hipStream_t s) {
  switch (dt) {
    case 0: return launch_batch_dt0(b, op, nSrcs, pol, grid, s);
    case 1: return launch_batch_dt1(b, op, nSrcs, pol, grid, s);
    case 2: return launch_batch_dt2(b, op, nSrcs, pol, grid, s);
    case 3: return launch_batch_dt3(b, op, nSrcs, pol, grid, s);
    case 4: return launch_batch_dt4(b, op, nSrcs, pol, grid, s);
    case 5: return launch_batch_dt5(b, op, nSrcs, pol, grid, s);
    case 6: return launch_batch_dt6(b, op, nSrcs, pol, grid, s);
    case 7: return launch_batch_dt7(b, op, nSrcs, pol, grid, s);
    case 8: return launch_batch_dt8(b, op, nSrcs, pol, grid, s);
    case 9: return launch_batch_dt9(b, op, nSrcs, pol, grid, s);
  }
  return hipErrorInvalidValue;
}

nexrResult_t launchSingle(const RCParams& p, int dt, int op, int nSrcs, hipStream_t stream, uint64_t maxGrid);

// One batch launch per run of <= kMaxBatch works that run the same kernel: the works as the semantics
// and the kernel routing (routeKernel) run them, grouped by (datatype, op, K, and for MinMax isMin),
// each group in order of first appearance. Work i gets max(1, workgroupsFor(work i)) workgroups (its
// one-shot grid), total capped at gridCap(block) by shrinking the largest shares (the kernel
// grid-strides inside each work's range). A run that would stream enough for non-temporal stores runs
// its works as single launches instead (kBatchPolicies, nexr_internal.h).
nexrResult_t reduceCopyBatch(const nexrReduceCopyWork* works, int nWorks, int datatype, int op, hipStream_t stream) {
  if (nWorks < 0 || (nWorks > 0 && works == nullptr)) return nexrInvalidArgument;
  for (int i = 0; i < nWorks; i++) {
    const nexrReduceCopyWork& w = works[i];
    nexrResult_t r = validate(w.nSrcs, w.srcs, w.nDsts, w.dsts, w.nElts, datatype, op, w.redOpArg, w.nPreOpSrcs,
                              w.preOpArgs);
    if (r != nexrSuccess) return r;
  }
  struct Routed {
    CallShape c;
    int minClass;  // MinMax: 1 = min ((redOpArg & 1) == 0), 0 = max
    size_t nElts;
    const nexrReduceCopyWork* w;
  };
  std::vector<Routed> rw;
  rw.reserve((size_t)nWorks);
  for (int i = 0; i < nWorks; i++) {
    const nexrReduceCopyWork& w = works[i];
    if (w.nElts == 0 || w.nDsts == 0) continue;
    Routed x{{datatype, op, w.nSrcs, w.nPreOpSrcs, w.postOp, nullptr}, 0, w.nElts, &w};
    applySemantics(x.c);
    routeKernel(x.c, &x.nElts);
    x.minClass = x.c.op == nexrDevMinMax && (w.redOpArg & 1) == 0 ? 1 : 0;
    rw.push_back(x);
  }
  std::vector<char> taken(rw.size(), 0);
  for (size_t i0 = 0; i0 < rw.size(); i0++) {
    if (taken[i0]) continue;
    const CallShape key = rw[i0].c;
    const int keyMin = rw[i0].minClass, k = key.nSrcs;
    const size_t esz = typeSize(key.dt);
    BatchParams b;
    b.nWorks = 0;
    uint64_t blocks[kMaxBatch];
    uint64_t streamBytes = 0;
    auto flush = [&]() -> nexrResult_t {
      if (b.nWorks == 0) return nexrSuccess;
      const int pol = pickPolicy(streamBytes);
      if (pol >= kBatchPolicies) {  // non-temporal stores: one launch per work, each at its own policy
        for (int i = 0; i < b.nWorks; i++) {
          nexrResult_t r = launchSingle(b.w[i], key.dt, key.op, k, stream, 0);
          if (r != nexrSuccess) return r;
        }
        b.nWorks = 0;
        streamBytes = 0;
        return nexrSuccess;
      }
      const int block = block_for(key.dt, k, pol);
      const uint64_t cap = gridCap(block);
      uint64_t total = 0;
      for (int i = 0; i < b.nWorks; i++) {
        const uint64_t need = workgroupsFor(b.w[i], k, key.dt, pol);
        blocks[i] = need < 1 ? 1 : (need < cap ? need : cap);
        total += blocks[i];
      }
      while (total > cap) {
        int big = 0;
        for (int i = 1; i < b.nWorks; i++)
          if (blocks[i] > blocks[big]) big = i;
        uint64_t cut = blocks[big] / 2;
        blocks[big] -= cut;
        total -= cut;
      }
      b.start[0] = 0;
      for (int i = 0; i < b.nWorks; i++) b.start[i + 1] = b.start[i] + (uint32_t)blocks[i];
      Geometry g;
      nexrResult_t r = pickGeometry(total, pol, block, &g);
      if (r != nexrSuccess) return r;
      NEXR_HIP(launchBatchDt(key.dt, b, key.op, k, g.pol, (int)total, stream));
      b.nWorks = 0;
      streamBytes = 0;
      return nexrSuccess;
    };
    for (size_t i = i0; i < rw.size(); i++) {
      const Routed& x = rw[i];
      if (taken[i] || x.c.dt != key.dt || x.c.op != key.op || x.c.nSrcs != k || x.minClass != keyMin) continue;
      taken[i] = 1;
      const nexrReduceCopyWork& w = *x.w;
      fillParams(b.w[b.nWorks], k, w.srcs, w.nDsts, w.dsts, x.nElts, esz, w.redOpArg, x.c.nPreOp, w.preOpArgs, nullptr,
                 x.c.postOp);
      streamBytes += (uint64_t)(k + w.nDsts) * x.nElts * esz;
      if (++b.nWorks == kMaxBatch) {
        nexrResult_t r = flush();
        if (r != nexrSuccess) return r;
      }
    }
    nexrResult_t r = flush();
    if (r != nexrSuccess) return r;
  }
  return nexrSuccess;
}

// One launch of a routed call whose parameters are filled: policy by the bytes it streams, one-shot grid
// (capped at maxGrid when > 0).
nexrResult_t launchSingle(const RCParams& p, int dt, int op, int nSrcs, hipStream_t stream, uint64_t maxGrid) {
  const uint64_t esz = (uint64_t)typeSize(dt);
  const int pol = pickPolicy((uint64_t)(nSrcs + p.nDsts) * p.nElts * esz, nSrcs, p.nDsts);
  uint64_t wgs = workgroupsFor(p, nSrcs, dt, pol);
  if (maxGrid > 0 && wgs > maxGrid) wgs = maxGrid;
  Geometry g;
  nexrResult_t r = pickGeometry(wgs, pol, block_for(dt, nSrcs, pol), &g);
  if (r != nexrSuccess) return r;
  NEXR_HIP(launchDt(dt, p, op, nSrcs, g, stream));
  return nexrSuccess;
}

// maxGrid > 0 caps the grid (the kernel grid-strides): launches that read or write host memory over
// PCIe use hostGrid() workgroups. With a one-shot grid every workgroup's loads are interleaved over the
// whole transfer, so every workgroup's last load lands near its end and the writes start only then;
// 32 workgroups keep ~1 MiB of reads in flight (more than the link's bandwidth x latency) and let the
// early workgroups write while the others still read: +4-9 % at 1 MiB, +10-20 % at 4 MiB and +6-12 % at
// 64 MiB per buffer over the one-shot grid (tools/zero_copy_sizes.py, profiles/r05f_zero_copy_grid.txt).
uint64_t hostGrid() {
  static const long g = envLong("NEXR_HOST_GRID", 32);
  return g > 0 ? (uint64_t)g : 0;
}

nexrResult_t reduceCopyDevice(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                              size_t nElts, int datatype, int op, uint64_t redOpArg, int nPreOpSrcs,
                              const uint64_t* preOpArgs, const void* prePtr, int postOp, hipStream_t stream,
                              uint64_t maxGrid = 0) {
  nexrResult_t r = validate(nSrcs, srcs, nDsts, dsts, nElts, datatype, op, redOpArg, nPreOpSrcs, preOpArgs);
  if (r != nexrSuccess) return r;
  if (nElts == 0 || nDsts == 0) return nexrSuccess;  // common_kernel.h:288-289: nothing to store
  CallShape c{datatype, op, nSrcs, nPreOpSrcs, postOp, prePtr};
  applySemantics(c);
  size_t n = nElts;
  routeKernel(c, &n);
  const size_t esz = typeSize(c.dt);
  RCParams p;
  fillParams(p, c.nSrcs, srcs, nDsts, dsts, n, esz, redOpArg, c.nPreOp, preOpArgs, c.prePtr, c.postOp);
  return launchSingle(p, c.dt, c.op, c.nSrcs, stream, maxGrid);
}

// ---- independent chunks on several GPUs from one host call -------------------
// One host thread per work: hipSetDevice, a stream of its own, the shared start barrier, `reps`
// launches, hipStreamSynchronize. A thread whose setup fails still arrives at the barrier (so the
// others are released) and reports its error.
// Streams come from a process-wide per-device pool: a stream is checked out for one work of one
// call and handed back drained. (A fresh stream per call cost ~1.5 ms on its first launches, which
// dominated calls of tens of MiB; profiles/r01s5_c_examples_gpu.txt.)
std::mutex gMdStreamMu;
std::vector<std::pair<int, hipStream_t>> gMdStreamIdle;
uint64_t gMdStreamsCreated = 0;  // under gMdStreamMu (nexrGetPoolStats)

hipError_t mdStreamTake(int dev, hipStream_t* st) {
  {
    std::lock_guard<std::mutex> g(gMdStreamMu);
    for (size_t i = 0; i < gMdStreamIdle.size(); i++)
      if (gMdStreamIdle[i].first == dev) {
        *st = gMdStreamIdle[i].second;
        gMdStreamIdle.erase(gMdStreamIdle.begin() + (long)i);
        return hipSuccess;
      }
  }
  hipError_t e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> g(gMdStreamMu);
    gMdStreamsCreated++;
  }
  return e;
}

void mdStreamGive(int dev, hipStream_t st) {  // st was synchronised without error
  std::lock_guard<std::mutex> g(gMdStreamMu);
  gMdStreamIdle.emplace_back(dev, st);
}
// nSets works per thread (works[i * nSets + s], all on devices[i]): launch k of thread i runs set
// k mod nSets, the rotation the N = 1 bench uses so no launch re-reads cache-resident bytes.
nexrResult_t reduceCopyMultiDevice(const nexrReduceCopyWork* works, const int* devices, int nWorks, int nSets,
                                   int datatype, int op, int reps, double* seconds) {
  if (nWorks < 0 || nWorks > NEXR_MAX_MULTI_DEVICE_WORKS || reps < 1) return nexrInvalidArgument;
  if (nSets < 1 || nSets > NEXR_MAX_MULTI_DEVICE_SETS) return nexrInvalidArgument;
  if (nWorks > 0 && (works == nullptr || devices == nullptr)) return nexrInvalidArgument;
  for (int i = 0; i < nWorks * nSets; i++) {
    const nexrReduceCopyWork& w = works[i];
    nexrResult_t r = validate(w.nSrcs, w.srcs, w.nDsts, w.dsts, w.nElts, datatype, op, w.redOpArg, w.nPreOpSrcs,
                              w.preOpArgs);
    if (r != nexrSuccess) return r;
  }
  if (seconds) *seconds = 0.0;
  if (nWorks == 0) return nexrSuccess;
  int nDev = 0;
  NEXR_HIP(hipGetDeviceCount(&nDev));
  for (int i = 0; i < nWorks; i++)
    if (devices[i] < 0 || devices[i] >= nDev) return nexrInvalidArgument;

  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  std::chrono::steady_clock::time_point t0;
  std::vector<std::chrono::steady_clock::time_point> t1(nWorks);
  std::vector<nexrResult_t> res(nWorks, nexrSuccess);
  std::vector<int> hipErr(nWorks, 0);
  bool cancel = false;  // set (under mu) when not every work got a thread: nothing runs
  auto run = [&](int i) {
    hipStream_t st = nullptr;
    hipError_t e = hipSetDevice(devices[i]);
    if (e == hipSuccess) e = mdStreamTake(devices[i], &st);
    if (e != hipSuccess) {
      res[i] = nexrUnhandledCudaError;
      hipErr[i] = (int)e;
    }
    {
      std::unique_lock<std::mutex> lk(mu);
      if (++arrived == nWorks) {
        t0 = std::chrono::steady_clock::now();
        cv.notify_all();
      } else {
        cv.wait(lk, [&] { return arrived == nWorks; });
      }
      if (cancel && res[i] == nexrSuccess) res[i] = nexrSystemError;
    }
    for (int k = 0; k < reps && res[i] == nexrSuccess; k++) {
      const nexrReduceCopyWork& w = works[(size_t)i * nSets + k % nSets];
      res[i] = reduceCopyDevice(w.nSrcs, w.srcs, w.nDsts, w.dsts, w.nElts, datatype, op, w.redOpArg, w.nPreOpSrcs,
                                w.preOpArgs, nullptr, w.postOp, st);
    }
    if (res[i] == nexrUnhandledCudaError && hipErr[i] == 0) hipErr[i] = tLastHipError;
    if (st) {
      e = hipStreamSynchronize(st);
      t1[i] = std::chrono::steady_clock::now();
      if (e != hipSuccess && res[i] == nexrSuccess) {
        res[i] = nexrUnhandledCudaError;
        hipErr[i] = (int)e;
      }
      if (e == hipSuccess) mdStreamGive(devices[i], st);
      else (void)hipStreamDestroy(st);
    } else {
      t1[i] = std::chrono::steady_clock::now();
    }
  };
  std::vector<std::thread> threads;
  bool spawnFailed = false;
  try {
    threads.reserve(nWorks);
    for (int i = 0; i < nWorks; i++) threads.emplace_back(run, i);
  } catch (...) {
    // A thread could not be created: the works that never got one count as arrived (so the started
    // threads leave the barrier), but none of them may run, and the call reports a system error.
    std::lock_guard<std::mutex> lk(mu);
    spawnFailed = true;
    cancel = true;
    for (int i = (int)threads.size(); i < nWorks; i++) res[i] = nexrSystemError;
    arrived += nWorks - (int)threads.size();
    if (arrived == nWorks) t0 = std::chrono::steady_clock::now();
    cv.notify_all();
  }
  for (auto& t : threads) t.join();
  if (spawnFailed) return nexrSystemError;
  for (int i = 0; i < nWorks; i++)
    if (res[i] != nexrSuccess) {
      tLastHipError = hipErr[i];
      return res[i];
    }
  if (seconds) {
    auto last = t1[0];
    for (int i = 1; i < nWorks; i++) last = t1[i] > last ? t1[i] : last;
    *seconds = std::chrono::duration<double>(last - t0).count();
  }
  return nexrSuccess;
}

// ---- host-staged variant: a process-wide pool of staging rings ----------------------------------
// A ring is two device slots of (K+1) x chunk bytes: chunk c is copied in (H2D) and reduced on the
// caller's stream while chunk c-1 is copied out (D2H) on the ring's own stream, so the two PCIe
// directions run concurrently. A call checks a ring out for its duration and hands it back, so the
// pool holds, per device, as many rings as host calls have ever run there at once. (The emulated
// collectives run each call's ranks on fresh threads: a ring cached per thread would be a new device
// allocation and stream per thread, never freed.)
struct HostStage {
  int device = -1;
  char* buf = nullptr;
  size_t slotBytes = 0;  // bytes per slot
  hipStream_t out = nullptr;
  hipEvent_t kernelDone[2] = {nullptr, nullptr};
  hipEvent_t outDone[2] = {nullptr, nullptr};
};
std::mutex gStageMu;
std::vector<HostStage*> gStageIdle;
uint64_t gStagesCreated = 0;  // under gStageMu (nexrGetPoolStats)

// Checks a ring out for the current device (the largest idle one, or a new one) and hands it back
// when the call ends. Release drains the ring's stream and the caller's stream first, so that no
// copy of this call still targets the slots when another call takes the ring; a ring whose streams
// report an error is dropped rather than reused.
struct StageLease {
  HostStage* st = nullptr;
  hipStream_t caller = nullptr;
  ~StageLease() {
    if (!st) return;
    bool ok = hipStreamSynchronize(st->out) == hipSuccess;
    ok = hipStreamSynchronize(caller) == hipSuccess && ok;
    if (!ok) {
      (void)hipGetLastError();
      return;
    }
    std::lock_guard<std::mutex> g(gStageMu);
    gStageIdle.push_back(st);
  }
};

nexrResult_t stageFor(size_t slotBytes, hipStream_t caller, StageLease* lease) {
  int dev = 0;
  NEXR_HIP(hipGetDevice(&dev));
  HostStage* st = nullptr;
  {
    std::lock_guard<std::mutex> g(gStageMu);
    size_t best = gStageIdle.size();
    for (size_t i = 0; i < gStageIdle.size(); i++)
      if (gStageIdle[i]->device == dev && (best == gStageIdle.size() || gStageIdle[i]->slotBytes > gStageIdle[best]->slotBytes))
        best = i;
    if (best < gStageIdle.size()) {
      st = gStageIdle[best];
      gStageIdle.erase(gStageIdle.begin() + (long)best);
    }
  }
  if (!st) {
    st = new HostStage();
    hipError_t e = hipStreamCreateWithFlags(&st->out, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
      e = hipEventCreateWithFlags(&st->kernelDone[i], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&st->outDone[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {  // free the half-built ring; it is never pooled
      for (int i = 0; i < 2; i++) {
        if (st->kernelDone[i]) (void)hipEventDestroy(st->kernelDone[i]);
        if (st->outDone[i]) (void)hipEventDestroy(st->outDone[i]);
      }
      if (st->out) (void)hipStreamDestroy(st->out);
      delete st;
      return hipFail(e);
    }
    st->device = dev;
    std::lock_guard<std::mutex> g(gStageMu);
    gStagesCreated++;
  }
  lease->st = st;
  lease->caller = caller;
  if (st->slotBytes < slotBytes) {  // idle ring: its stream was drained when it was handed back
    if (st->buf) NEXR_HIP(hipFree(st->buf));
    st->buf = nullptr;
    st->slotBytes = 0;
    NEXR_HIP(hipMalloc((void**)&st->buf, 2 * slotBytes));
    st->slotBytes = slotBytes;
  }
  return nexrSuccess;
}

// hipMemcpyAsync between device memory and `bytes` of a host buffer that begins inside a pinned range the runtime
// knows (hipHostRegister, hipHostMalloc) and may run past its end: the runtime refuses such a copy whole
// (hipErrorInvalidValue: it finds the range by the host pointer and the copy does not fit it), so it is made in
// pieces, each ending where the range that holds its first byte ends; a piece that begins in memory the runtime
// does not know is an ordinary pageable copy to the buffer's end.
hipError_t hostCopyPieces(char* dev, char* host, size_t bytes, bool toDevice, hipStream_t s) {
  while (bytes > 0) {
    size_t piece = bytes;
    uintptr_t beg = 0;
    size_t size = 0;
    if (hipPointerGetAttribute(&beg, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)host) == hipSuccess &&
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)host) == hipSuccess &&
        (uintptr_t)host >= beg && (uintptr_t)host < beg + size) {
      if (beg + size - (uintptr_t)host < piece) piece = beg + size - (uintptr_t)host;
    } else {
      (void)hipGetLastError();  // pageable memory reports an error: not a failure of this call
    }
    const hipError_t e = toDevice ? hipMemcpyAsync(dev, host, piece, hipMemcpyHostToDevice, s)
                                  : hipMemcpyAsync(host, dev, piece, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    dev += piece;
    host += piece;
    bytes -= piece;
  }
  return hipSuccess;
}

// ---- host-staged variant, large pageable calls: a CPU copy team and pinned zero-copy slots -------
// The runtime's pageable hipMemcpyAsync copies through its own staging buffer with one CPU memcpy
// before each DMA, which held the C2 mix to 49 GB/s against an ~86 GB/s PCIe floor
// (profiles/r01_h2d_probe.log). For a call with at least NEXR_HOST_MT_MIN_BYTES of pageable
// buffers: a team of host threads copies each chunk of the pageable sources into a pinned,
// device-mapped slot; the kernel reads the slot and writes its output slot in place over PCIe
// (zero-copy, both link directions at once; pinned user buffers are read/written in place as
// well); the team copies the output slot to the pageable destinations. Three slots: chunk c is
// filled while chunk c-1 is reduced and chunk c-2 is drained.
constexpr int kPinnedSlots = 3;
struct PinnedStage {
  int device = -1;
  char* host = nullptr;  // hipHostMalloc (pinned, mapped, coherent): kPinnedSlots x slotBytes
  char* dev = nullptr;   // the same bytes as the device addresses them
  size_t slotBytes = 0;
  hipEvent_t done[kPinnedSlots] = {};
};
std::mutex gPinMu;
std::vector<PinnedStage*> gPinIdle;
uint64_t gPinCreated = 0;  // under gPinMu (nexrGetPoolStats)

// Checks a pinned ring out for the current device; the lease drains the caller's stream (every
// kernel this call queued, even one whose completion event could not be recorded) and every slot's
// event before handing the ring back; a ring that reports an error is dropped, not reused.
struct PinLease {
  PinnedStage* st = nullptr;
  hipStream_t caller = nullptr;
  ~PinLease() {
    if (!st) return;
    bool ok = hipStreamSynchronize(caller) == hipSuccess;
    for (int i = 0; i < kPinnedSlots; i++) ok = hipEventSynchronize(st->done[i]) == hipSuccess && ok;
    if (!ok) {
      (void)hipGetLastError();
      return;
    }
    std::lock_guard<std::mutex> g(gPinMu);
    gPinIdle.push_back(st);
  }
};

nexrResult_t pinnedFor(size_t slotBytes, hipStream_t caller, PinLease* lease) {
  int dev = 0;
  NEXR_HIP(hipGetDevice(&dev));
  PinnedStage* st = nullptr;
  {
    std::lock_guard<std::mutex> g(gPinMu);
    for (size_t i = 0; i < gPinIdle.size(); i++)
      if (gPinIdle[i]->device == dev && (!st || gPinIdle[i]->slotBytes > st->slotBytes)) st = gPinIdle[i];
    if (st) gPinIdle.erase(std::find(gPinIdle.begin(), gPinIdle.end(), st));
  }
  if (!st) {
    st = new PinnedStage();
    hipError_t e = hipSuccess;
    for (int i = 0; i < kPinnedSlots && e == hipSuccess; i++)
      e = hipEventCreateWithFlags(&st->done[i], hipEventDisableTiming);
    if (e == hipSuccess) {  // the events start "complete": record each once on the null stream
      for (int i = 0; i < kPinnedSlots && e == hipSuccess; i++) e = hipEventRecord(st->done[i], nullptr);
    }
    if (e != hipSuccess) {
      for (int i = 0; i < kPinnedSlots; i++)
        if (st->done[i]) (void)hipEventDestroy(st->done[i]);
      delete st;
      return hipFail(e);
    }
    st->device = dev;
    std::lock_guard<std::mutex> g(gPinMu);
    gPinCreated++;
  }
  lease->st = st;
  lease->caller = caller;
  if (st->slotBytes < slotBytes) {  // idle ring: its events were synchronised when it was handed back
    if (st->host) NEXR_HIP(hipHostFree(st->host));
    st->host = st->dev = nullptr;
    st->slotBytes = 0;
    NEXR_HIP(hipHostMalloc((void**)&st->host, kPinnedSlots * slotBytes, hipHostMallocDefault));
    NEXR_HIP(hipHostGetDevicePointer((void**)&st->dev, st->host, 0));
    st->slotBytes = slotBytes;
  }
  return nexrSuccess;
}

// Parallel memcpy: `run` splits every task into one contiguous, 4 KiB-aligned piece per thread and
// returns when all pieces are copied. The calling thread copies a piece too; the others are
// created for one host call and joined when it ends.
class CopyTeam {
 public:
  struct Task {
    char* dst;
    const char* src;
    size_t bytes;
  };
  explicit CopyTeam(int n) {
    for (int i = 1; i < n; i++) {
      try {
        workers_.emplace_back([this, i] { loop(i); });
      } catch (...) {  // fewer threads than asked for: the pieces are re-split over those that exist
        break;
      }
    }
    n_ = 1 + (int)workers_.size();
  }
  ~CopyTeam() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  void run(const Task* tasks, int nTasks) {
    {
      std::lock_guard<std::mutex> g(mu_);
      tasks_ = tasks;
      nTasks_ = nTasks;
      pending_ = n_ - 1;
      gen_++;
    }
    cv_.notify_all();
    piece(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return pending_ == 0; });
  }

 private:
  void piece(int idx) const {
    for (int t = 0; t < nTasks_; t++) {
      const Task& k = tasks_[t];
      const size_t per = ((k.bytes + n_ - 1) / n_ + 4095) & ~(size_t)4095;
      const size_t b0 = per * (size_t)idx;
      if (b0 >= k.bytes) continue;
      memcpy(k.dst + b0, k.src + b0, per < k.bytes - b0 ? per : k.bytes - b0);
    }
  }
  void loop(int idx) {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
      }
      piece(idx);
      std::lock_guard<std::mutex> g(mu_);
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> workers_;
  int n_ = 1;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  uint64_t gen_ = 0;
  int pending_ = 0;
  bool stop_ = false;
  const Task* tasks_ = nullptr;
  int nTasks_ = 0;
};

// srcs/dsts: the caller's host pointers; psrc/pdst: which are pinned (zsrc/zdst: their device
// addresses, used in place).
nexrResult_t reduceCopyHostTeam(int nSrcs, const void* const* srcs, const bool* psrc, const void* const* zsrc,
                                int nDsts, void* const* dsts, const bool* pdst, void* const* zdst, size_t nElts,
                                int datatype, int op, uint64_t redOpArg, int nPreOpSrcs, const uint64_t* preOpArgs,
                                int postOp, hipStream_t s, int nThreads) {
  const size_t esz = typeSize(datatype);
  // A team's chunk is an eighth of a buffer, between 4 MiB and NEXR_HOST_MT_CHUNK_BYTES (32 MiB), so
  // that a call runs at least 8 chunks through the 3 slots; alone, NEXR_HOST_SMALL_CHUNK_BYTES (4 MiB).
  static const long chunkTeam = envLong("NEXR_HOST_MT_CHUNK_BYTES", 32l << 20);
  static const long chunkSolo = envLong("NEXR_HOST_SMALL_CHUNK_BYTES", 4l << 20);
  long chunkOverride = chunkSolo;
  if (nThreads > 1) {
    const long eighth = (long)(nElts * esz / 8);
    chunkOverride = eighth < (4l << 20) ? (4l << 20) : eighth;
    if (chunkOverride > chunkTeam) chunkOverride = chunkTeam;
  }
  size_t chunkElts = ((size_t)(chunkOverride > 4096 ? chunkOverride : 4096) / esz) & ~(size_t)15;
  if (chunkElts > nElts) chunkElts = nElts;
  const size_t chunkBytes = ((chunkElts * esz) + 4095) & ~(size_t)4095;
  int nPageSrc = 0;
  bool outStaged = false;
  for (int k = 0; k < nSrcs; k++) nPageSrc += psrc[k] ? 0 : 1;
  for (int d = 0; d < nDsts; d++) outStaged |= !pdst[d];
  PinLease lease;
  nexrResult_t r = pinnedFor(chunkBytes * (size_t)(nPageSrc + (outStaged ? 1 : 0)), s, &lease);
  if (r != nexrSuccess) return r;
  PinnedStage* st = lease.st;
  CopyTeam team(nThreads);
  const size_t nChunks = (nElts + chunkElts - 1) / chunkElts;
  auto span = [&](size_t c, size_t* e0, size_t* n) {
    *e0 = c * chunkElts;
    *n = nElts - *e0 < chunkElts ? nElts - *e0 : chunkElts;
  };
  auto outOffset = [&] { return chunkBytes * (size_t)nPageSrc; };
  // Copy-in tasks of chunk c (its pageable sources into slot c % 3) and copy-out tasks of chunk c
  // (slot c % 3's output to the pageable destinations), appended to `tasks`.
  CopyTeam::Task tasks[NEXR_MAX_SRCS + NEXR_MAX_DSTS];
  int nTasks = 0;
  auto copyIn = [&](size_t c) {
    size_t e0, n;
    span(c, &e0, &n);
    const size_t slot = (c % kPinnedSlots) * st->slotBytes;
    for (int k = 0, j = 0; k < nSrcs; k++)
      if (!psrc[k]) tasks[nTasks++] = {st->host + slot + chunkBytes * j++, (const char*)srcs[k] + e0 * esz, n * esz};
  };
  auto copyOut = [&](size_t c) {
    size_t e0, n;
    span(c, &e0, &n);
    const char* out = st->host + (c % kPinnedSlots) * st->slotBytes + outOffset();
    for (int d = 0; d < nDsts; d++)
      if (!pdst[d]) tasks[nTasks++] = {(char*)dsts[d] + e0 * esz, out, n * esz};
  };
  auto launch = [&](size_t c) -> nexrResult_t {
    size_t e0, n;
    span(c, &e0, &n);
    const size_t slot = (c % kPinnedSlots) * st->slotBytes;
    const void* dsrc[NEXR_MAX_SRCS];
    for (int k = 0, j = 0; k < nSrcs; k++)
      dsrc[k] = psrc[k] ? (const void*)((const char*)zsrc[k] + e0 * esz) : (const void*)(st->dev + slot + chunkBytes * j++);
    void* ddst[NEXR_MAX_DSTS + 1];
    int m = 0;
    for (int d = 0; d < nDsts; d++)
      if (pdst[d]) ddst[m++] = (char*)zdst[d] + e0 * esz;
    if (outStaged) ddst[m++] = st->dev + slot + outOffset();
    nexrResult_t rr = reduceCopyDevice(nSrcs, dsrc, m, ddst, n, datatype, op, redOpArg, nPreOpSrcs, preOpArgs,
                                       nullptr, postOp, s, hostGrid());
    if (rr != nexrSuccess) return rr;
    NEXR_HIP(hipEventRecord(st->done[c % kPinnedSlots], s));
    return nexrSuccess;
  };
  // Iteration c: wait for chunk c-2's kernel, then ONE team pass copies chunk c-2's output out of
  // slot (c-2) % 3 and chunk c's sources into slot c % 3 (drained one iteration ago) while the GPU
  // reduces chunk c-1; then chunk c's kernel is queued.
  for (size_t c = 0; c < nChunks + 2; c++) {
    nTasks = 0;
    uint64_t t0 = nowNs();
    if (c >= 2) {
      NEXR_HIP(hipEventSynchronize(st->done[(c - 2) % kPinnedSlots]));
      const uint64_t t1 = nowNs();
      gHpWaitNs.fetch_add(t1 - t0, std::memory_order_relaxed);
      t0 = t1;
      if (outStaged) copyOut(c - 2);
    }
    if (c < nChunks) copyIn(c);
    if (nTasks > 0) team.run(tasks, nTasks);
    const uint64_t t1 = nowNs();
    gHpCopyNs.fetch_add(t1 - t0, std::memory_order_relaxed);
    if (c < nChunks) {
      r = launch(c);
      if (r != nexrSuccess) return r;
      gHpLaunchNs.fetch_add(nowNs() - t1, std::memory_order_relaxed);
    }
  }
  return nexrSuccess;
}

// ---- host-side half/bfloat16 rounding used by the op encoder (RNE, NaN -> 0x7fff) ------------
uint16_t floatToHalfRne(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const uint32_t a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return 0x7fffu;
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to +-inf
  if (a < 0x33000001u) return (uint16_t)sign;               // <= 2^-25 rounds to 0
  uint32_t mant, shift;
  if (a >= 0x38800000u) {  // normal half
    mant = a - 0x38000000u;
    shift = 13;
  } else {  // subnormal half
    const uint32_t e = a >> 23;
    mant = (a & 0x7fffffu) | 0x800000u;
    shift = 126 - e;
  }
  uint32_t q = mant >> shift;
  const uint32_t rem = mant & ((1u << shift) - 1);
  const uint32_t halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (q & 1))) q++;
  return (uint16_t)(sign | q);
}
uint16_t floatToBf16Rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fffu;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// ---- host registration cache (reference: ncclCommRegister's per-comm regCache, sorted by begin
// address, src/register/register.cc:40-60; ncclMemAlloc, src/allocator.cc:11-) -----------------
// Pinned, device-mapped host ranges the library registered (nexrHostRegister) or allocated
// (nexrHostMemAlloc), sorted by begin address. nexrReduceCopyHost looks a buffer up here first, so a
// call on registered memory costs no HIP query per buffer; because the library made every entry, it
// also knows when one ends (nexrHostDeregister / nexrHostMemFree), so nothing here goes stale.
// Entries hold exact byte ranges. hipHostRegister pins every page a range touches, and on this ROCm it
// accepts a second range that shares a page with a registered one (adjacent heap buffers do, e.g. the
// C1 bench's numpy arrays), giving it a mapping of its own, so such neighbours are separate entries
// whose deregistrations are independent (tests/test_host_register_gpu.py); should the runtime refuse
// one, the call returns nexrInvalidUsage, not a raw HIP error. Handles are monotonic ids, never
// addresses: a handle whose entry is gone stays invalid even when a later entry lands at the same
// address.
struct HostReg {
  uintptr_t beg = 0, end = 0;
  char* dev = nullptr;         // device address of beg
  void* hipPtr = nullptr;      // the pointer hipHostRegister / hipHostMalloc returned or took
  bool owned = false;          // allocated by nexrHostMemAlloc (freed by nexrHostMemFree), else registered
  int regs = 0;                // live nexrHostRegister references to this entry (its handles)
  uint64_t id = 0;
};
std::shared_mutex gRegMu;
std::vector<HostReg*> gRegs;  // sorted by beg, non-overlapping
uint64_t gRegNextId = 1;      // under gRegMu

uintptr_t pageSize() {
  static const uintptr_t ps = [] {
    const long v = sysconf(_SC_PAGESIZE);
    return (uintptr_t)(v > 0 ? v : 4096);
  }();
  return ps;
}
uintptr_t pageFloor(uintptr_t a) { return a & ~(pageSize() - 1); }
uintptr_t pageCeil(uintptr_t a) { return (a + pageSize() - 1) & ~(pageSize() - 1); }

// The device address of [p, p + bytes) when the whole range lies inside one entry.
bool regLookup(const void* p, size_t bytes, void** dev) {
  const uintptr_t a = (uintptr_t)p;
  std::shared_lock<std::shared_mutex> lk(gRegMu);
  auto it = std::upper_bound(gRegs.begin(), gRegs.end(), a, [](uintptr_t v, const HostReg* r) { return v < r->beg; });
  if (it == gRegs.begin()) return false;
  const HostReg* r = *(it - 1);
  if (a + bytes > r->end || a + bytes < a) return false;
  *dev = r->dev + (a - r->beg);
  return true;
}

// Index of the entry containing [a, a + n), -1 if none; overlap: some entry intersects it; sharesPage:
// some entry shares a page with it.
int regFind(uintptr_t a, size_t n, bool* overlap, bool* sharesPage) {
  *overlap = *sharesPage = false;
  const uintptr_t pb = pageFloor(a), pe = pageCeil(a + n);
  for (size_t i = 0; i < gRegs.size(); i++) {
    const HostReg* r = gRegs[i];
    if (a >= r->beg && a + n <= r->end) return (int)i;
    if (a < r->end && a + n > r->beg) *overlap = true;
    if (pb < pageCeil(r->end) && pe > pageFloor(r->beg)) *sharesPage = true;
  }
  return -1;
}

void regInsert(HostReg* r) {
  r->id = gRegNextId++;
  auto it = std::upper_bound(gRegs.begin(), gRegs.end(), r->beg, [](uintptr_t v, const HostReg* x) { return v < x->beg; });
  gRegs.insert(it, r);
}

std::vector<HostReg*>::iterator regById(const void* handle) {
  const uint64_t id = (uint64_t)(uintptr_t)handle;
  return std::find_if(gRegs.begin(), gRegs.end(), [&](const HostReg* r) { return r->id == id; });
}

}  // namespace
}  // namespace nexr

using namespace nexr;

extern "C" {

NEXR_API nexrResult_t nexrReduceCopy(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                     size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                     int nPreOpSrcs, const uint64_t* preOpArgs, int postOp,
                                     nexrStream_t stream) {
  return reduceCopyDevice(nSrcs, srcs, nDsts, dsts, nElts, datatype, devRedOp, redOpArg, nPreOpSrcs,
                          preOpArgs, nullptr, postOp, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrGetPoolStats(uint64_t* multiDeviceStreams, uint64_t* hostStagingRings) {
  if (multiDeviceStreams) {
    std::lock_guard<std::mutex> g(gMdStreamMu);
    *multiDeviceStreams = gMdStreamsCreated;
  }
  if (hostStagingRings) {
    uint64_t n = 0;
    {
      std::lock_guard<std::mutex> g(gStageMu);
      n = gStagesCreated;
    }
    std::lock_guard<std::mutex> g(gPinMu);
    *hostStagingRings = n + gPinCreated;
  }
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrQueryLaunch(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                      size_t nElts, int datatype, nexrLaunchInfo* info) {
  if (info == nullptr) return nexrInvalidArgument;
  memset(info, 0, sizeof(*info));
  nexrResult_t r = validate(nSrcs, srcs, nDsts, dsts, nElts, datatype, nexrDevSum, 0, 0, nullptr);
  if (r != nexrSuccess) return r;
  if (nElts == 0 || nDsts == 0) return nexrSuccess;  // nothing would be launched
  CallShape c{datatype, nexrDevSum, nSrcs, 0, 0, nullptr};
  applySemantics(c);
  routeKernel(c, &nElts);  // a K = 1 call is a byte copy: headElts / bodyPacks of the uint8 kernel
  nSrcs = c.nSrcs;
  datatype = c.dt;
  const size_t esz = typeSize(datatype);
  RCParams p;
  fillParams(p, nSrcs, srcs, nDsts, dsts, nElts, esz, 0, 0, nullptr, nullptr, 0);
  Geometry g;
  const int pol = pickPolicy((uint64_t)(nSrcs + nDsts) * nElts * esz, nSrcs, nDsts);
  const int block = block_for(datatype, nSrcs, pol);
  r = pickGeometry(workgroupsFor(p, nSrcs, datatype, pol), pol, block, &g);
  if (r != nexrSuccess) return r;
  info->grid = (uint32_t)g.grid;
  info->block = block;
  info->packsPerLane = unroll_for(datatype, nSrcs, pol);
  info->policy = g.pol;
  info->unaligned = p.unaligned;
  info->headElts = p.head;
  info->bodyPacks = p.nPacks;
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrReduceCopyBatch(const nexrReduceCopyWork* works, int nWorks, int datatype, int devRedOp,
                                          nexrStream_t stream) {
  return reduceCopyBatch(works, nWorks, datatype, devRedOp, (hipStream_t)stream);
}

NEXR_API nexrResult_t nexrReduceCopyMultiDevice(const nexrReduceCopyWork* works, const int* devices, int nWorks,
                                                int datatype, int devRedOp, int reps, double* seconds) {
  return reduceCopyMultiDevice(works, devices, nWorks, 1, datatype, devRedOp, reps, seconds);
}
NEXR_API nexrResult_t nexrReduceCopyMultiDeviceSets(const nexrReduceCopyWork* works, const int* devices, int nWorks,
                                                    int nSets, int datatype, int devRedOp, int reps, double* seconds) {
  return reduceCopyMultiDevice(works, devices, nWorks, nSets, datatype, devRedOp, reps, seconds);
}

NEXR_API nexrResult_t nexrReduceCopyHost(int nSrcs, const void* const* srcs, int nDsts, void* const* dsts,
                                         size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                         int nPreOpSrcs, const uint64_t* preOpArgs, int postOp,
                                         nexrStream_t stream) {
  nexrResult_t r = validate(nSrcs, srcs, nDsts, dsts, nElts, datatype, devRedOp, redOpArg, nPreOpSrcs, preOpArgs);
  if (r != nexrSuccess) return r;
  if (nElts == 0 || nDsts == 0) return nexrSuccess;
  hipStream_t s = (hipStream_t)stream;
  // Zero-copy: when every buffer is pinned (page-locked, device-mapped) host memory the kernel reads
  // and writes it directly over PCIe, both directions at once, with no staging copies (measured
  // 80.7 GB/s vs 71.5 GB/s staged for the C2 mix: profiles/r01_h2d_probe.log).
  const void* zsrc[NEXR_MAX_SRCS];
  void* zdst[NEXR_MAX_DSTS];
  bool psrc[NEXR_MAX_SRCS], pdst[NEXR_MAX_DSTS];  // pinned (device-mapped) buffers
  // begins inside a pinned range and runs past its end: staged, and by the runtime only in pieces (hostCopyPieces)
  bool csrc[NEXR_MAX_SRCS] = {}, cdst[NEXR_MAX_DSTS] = {};
  // Classification: the registration cache first (no HIP call); otherwise the runtime's pointer
  // query, trusted only when the whole buffer lies inside the pinned range it reports.
  static const long zeroCopy = envLong("NEXR_HOST_ZERO_COPY", 1);
  const size_t esz = typeSize(datatype);
  const size_t bufBytes = nElts * esz;
  const uint64_t tc0 = nowNs();
  gHpCalls.fetch_add(1, std::memory_order_relaxed);
  int nPinned = 0;
  for (int k = 0; k < nSrcs + nDsts; k++) {
    const void* hp = k < nSrcs ? srcs[k] : dsts[k - nSrcs];
    void* dev = nullptr;
    bool pin = false, cut = false;
    if (zeroCopy != 0) {
      if (regLookup(hp, bufBytes, &dev)) {
        pin = true;
        gHpRegHits.fetch_add(1, std::memory_order_relaxed);
      } else {
        gHpQueries.fetch_add(1, std::memory_order_relaxed);
        hipPointerAttribute_t a;
        pin = hipPointerGetAttributes(&a, hp) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer != nullptr;
        if (pin) {
          dev = a.devicePointer;
          // A pointer inside a registered range whose buffer runs past its end must not be read in
          // place: the device mapping covers only the range. Without the range, nothing is.
          uintptr_t beg = 0;
          size_t size = 0;
          if (hipPointerGetAttribute(&beg, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)hp) != hipSuccess ||
              hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)hp) != hipSuccess ||
              (uintptr_t)hp < beg || (uintptr_t)hp + bufBytes > beg + size) {
            pin = false;
            cut = true;
          }
        }
        (void)hipGetLastError();  // pageable memory reports an error: not a failure of this call
      }
    }
    if (k < nSrcs) {
      psrc[k] = pin;
      csrc[k] = cut;
      zsrc[k] = pin ? dev : nullptr;
    } else {
      pdst[k - nSrcs] = pin;
      cdst[k - nSrcs] = cut;
      zdst[k - nSrcs] = pin ? dev : nullptr;
    }
    nPinned += pin ? 1 : 0;
  }
  const uint64_t tc1 = nowNs();
  gHpClassifyNs.fetch_add(tc1 - tc0, std::memory_order_relaxed);
  if (nPinned == nSrcs + nDsts) {
    gHpZeroCopy.fetch_add(1, std::memory_order_relaxed);
    r = reduceCopyDevice(nSrcs, zsrc, nDsts, zdst, nElts, datatype, devRedOp, redOpArg, nPreOpSrcs, preOpArgs,
                         nullptr, postOp, s, hostGrid());
    const uint64_t tc2 = nowNs();
    gHpLaunchNs.fetch_add(tc2 - tc1, std::memory_order_relaxed);
    if (r != nexrSuccess) return r;
    NEXR_HIP(hipStreamSynchronize(s));
    gHpWaitNs.fetch_add(nowNs() - tc2, std::memory_order_relaxed);
    return nexrSuccess;
  }
  // Pageable buffers, by the pageable bytes the call moves (profiles/r02_host_sizes_sweep.log):
  //   <= NEXR_HOST_SOLO_MAX_BYTES (4 MiB; the emulated ring's slices): the calling thread copies them
  //      into pinned zero-copy slots (reduceCopyHostTeam, one thread): 1.2-1.9x the runtime copies;
  //   >= NEXR_HOST_MT_MIN_BYTES (256 MiB): a team of NEXR_HOST_COPY_THREADS (8) threads does: 1.1-1.2x;
  //   in between, and always with NEXR_HOST_COPY_THREADS=0: the runtime-copy chunk pipeline below,
  //      which is as fast or faster there.
  static const long mtMin = envLong("NEXR_HOST_MT_MIN_BYTES", 256l << 20);
  static const long soloMax = envLong("NEXR_HOST_SOLO_MAX_BYTES", 4l << 20);
  static const long mtThreads = envLong("NEXR_HOST_COPY_THREADS", 8);
  const uint64_t pageable = (uint64_t)(nSrcs + nDsts - nPinned) * nElts * esz;
  if (mtThreads >= 1 && (pageable >= (uint64_t)mtMin || pageable <= (uint64_t)soloMax)) {
    const bool large = pageable >= (uint64_t)mtMin;
    return reduceCopyHostTeam(nSrcs, srcs, psrc, zsrc, nDsts, dsts, pdst, zdst, nElts, datatype, devRedOp, redOpArg,
                              nPreOpSrcs, preOpArgs, postOp, s, large ? (int)(mtThreads > 64 ? 64 : mtThreads) : 1);
  }
  // Some buffers pageable: a two-stream chunk pipeline through device memory for those only; the
  // pinned ones (e.g. the emulated transport's FIFOs) are read and written in place by the kernel.
  static const long chunkOverride = envLong("NEXR_HOST_CHUNK_BYTES", 8l << 20);
  size_t chunkElts = ((size_t)(chunkOverride > 4096 ? chunkOverride : 4096) / esz) & ~(size_t)15;
  if (chunkElts > nElts) chunkElts = nElts;
  const size_t chunkBytes = ((chunkElts * esz) + 255) & ~(size_t)255;
  StageLease lease;
  r = stageFor(chunkBytes * (size_t)(nSrcs + 1), s, &lease);
  if (r != nexrSuccess) return r;
  HostStage* st = lease.st;
  bool anyPageableDst = false;
  for (int d = 0; d < nDsts; d++) anyPageableDst |= !pdst[d];
  const size_t nChunks = (nElts + chunkElts - 1) / chunkElts;
  const uint64_t tp = nowNs();
  for (size_t c = 0; c < nChunks; c++) {
    const int slot = (int)(c & 1);
    const size_t e0 = c * chunkElts;
    const size_t n = (nElts - e0 < chunkElts) ? nElts - e0 : chunkElts;
    char* base = st->buf + (size_t)slot * st->slotBytes;
    if (c >= 2) NEXR_HIP(hipStreamWaitEvent(s, st->outDone[slot], 0));  // slot drained by chunk c-2's D2H
    const void* dsrc[NEXR_MAX_SRCS];
    for (int k = 0; k < nSrcs; k++) {
      if (psrc[k]) {
        dsrc[k] = (const char*)zsrc[k] + e0 * esz;
        continue;
      }
      dsrc[k] = base + chunkBytes * k;
      if (csrc[k])
        NEXR_HIP(hostCopyPieces((char*)dsrc[k], (char*)srcs[k] + e0 * esz, n * esz, true, s));
      else
        NEXR_HIP(hipMemcpyAsync((void*)dsrc[k], (const char*)srcs[k] + e0 * esz, n * esz, hipMemcpyHostToDevice, s));
    }
    void* ddst[NEXR_MAX_DSTS + 1];
    int m = 0;
    for (int d = 0; d < nDsts; d++)
      if (pdst[d]) ddst[m++] = (char*)zdst[d] + e0 * esz;
    char* staged = base + chunkBytes * nSrcs;
    if (anyPageableDst) ddst[m++] = staged;
    r = reduceCopyDevice(nSrcs, dsrc, m, ddst, n, datatype, devRedOp, redOpArg, nPreOpSrcs, preOpArgs, nullptr,
                         postOp, s, nPinned > 0 ? hostGrid() : 0);
    if (r != nexrSuccess) return r;
    NEXR_HIP(hipEventRecord(st->kernelDone[slot], s));
    NEXR_HIP(hipStreamWaitEvent(st->out, st->kernelDone[slot], 0));
    for (int d = 0; d < nDsts; d++) {
      if (pdst[d]) continue;
      if (cdst[d])
        NEXR_HIP(hostCopyPieces(staged, (char*)dsts[d] + e0 * esz, n * esz, false, st->out));
      else
        NEXR_HIP(hipMemcpyAsync((char*)dsts[d] + e0 * esz, staged, n * esz, hipMemcpyDeviceToHost, st->out));
    }
    NEXR_HIP(hipEventRecord(st->outDone[slot], st->out));
  }
  const uint64_t tw = nowNs();
  gHpLaunchNs.fetch_add(tw - tp, std::memory_order_relaxed);
  NEXR_HIP(hipStreamSynchronize(st->out));
  NEXR_HIP(hipStreamSynchronize(s));
  gHpWaitNs.fetch_add(nowNs() - tw, std::memory_order_relaxed);
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrHostRegister(void* buff, size_t size, void** handle) {
  if (buff == nullptr || size == 0 || handle == nullptr) return nexrInvalidArgument;
  const uintptr_t a = (uintptr_t)buff;
  if (a + size < a) return nexrInvalidArgument;
  std::unique_lock<std::shared_mutex> lk(gRegMu);
  bool overlap = false, sharesPage = false;
  const int i = regFind(a, size, &overlap, &sharesPage);
  if (i >= 0) {  // inside a range this library already maps (registered or allocated): share it (register.cc:49-76)
    gRegs[i]->regs++;
    *handle = (void*)(uintptr_t)gRegs[i]->id;
    return nexrSuccess;
  }
  if (overlap) return nexrInvalidUsage;  // partly inside another entry: hipHostRegister would refuse it
  hipError_t e = hipHostRegister(buff, size, hipHostRegisterMapped | hipHostRegisterPortable);
  if (e != hipSuccess) {
    if (sharesPage) {  // a page-sharing neighbour the runtime refused: the documented usage error
      (void)hipGetLastError();
      return nexrInvalidUsage;
    }
    return hipFail(e);
  }
  void* dev = nullptr;
  e = hipHostGetDevicePointer(&dev, buff, 0);
  if (e != hipSuccess) {
    (void)hipHostUnregister(buff);
    return hipFail(e);
  }
  HostReg* r = new HostReg();
  r->beg = a;
  r->end = a + size;
  r->dev = (char*)dev;
  r->hipPtr = buff;
  r->regs = 1;
  regInsert(r);
  *handle = (void*)(uintptr_t)r->id;
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrHostDeregister(void* handle) {
  if (handle == nullptr) return nexrSuccess;  // ncclCommDeregister accepts a NULL handle
  std::unique_lock<std::shared_mutex> lk(gRegMu);
  auto it = regById(handle);
  if (it == gRegs.end() || (*it)->regs == 0) return nexrInvalidUsage;  // register.cc:150-153
  HostReg* r = *it;
  if (--r->regs > 0 || r->owned) return nexrSuccess;  // an allocation's pages stay until nexrHostMemFree
  gRegs.erase(it);
  hipError_t e = hipHostUnregister(r->hipPtr);
  delete r;
  NEXR_HIP(e);
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrHostMemAlloc(void** ptr, size_t size) {
  if (ptr == nullptr || size == 0) return nexrInvalidArgument;
  *ptr = nullptr;
  void* host = nullptr;
  NEXR_HIP(hipHostMalloc(&host, size, hipHostMallocMapped | hipHostMallocPortable));
  void* dev = nullptr;
  hipError_t e = hipHostGetDevicePointer(&dev, host, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(host);
    return hipFail(e);
  }
  HostReg* r = new HostReg();
  r->beg = (uintptr_t)host;
  r->end = (uintptr_t)host + size;
  r->dev = (char*)dev;
  r->hipPtr = host;
  r->owned = true;
  std::unique_lock<std::shared_mutex> lk(gRegMu);
  regInsert(r);
  *ptr = host;
  return nexrSuccess;
}

// Refused (nexrInvalidUsage) while registrations inside the allocation remain: their handles would
// otherwise name freed memory (the caller deregisters first, as ncclCommDeregister before ncclMemFree).
NEXR_API nexrResult_t nexrHostMemFree(void* ptr) {
  if (ptr == nullptr) return nexrSuccess;
  std::unique_lock<std::shared_mutex> lk(gRegMu);
  auto it = std::find_if(gRegs.begin(), gRegs.end(), [&](const HostReg* r) { return r->owned && r->hipPtr == ptr; });
  if (it == gRegs.end()) return nexrInvalidArgument;
  HostReg* r = *it;
  if (r->regs > 0) return nexrInvalidUsage;
  gRegs.erase(it);
  delete r;
  NEXR_HIP(hipHostFree(ptr));
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrGetHostPathStats(nexrHostPathStats* stats, int reset) {
  if (stats == nullptr) return nexrInvalidArgument;
  auto take = [&](std::atomic<uint64_t>& a) { return reset ? a.exchange(0) : a.load(); };
  stats->calls = take(gHpCalls);
  stats->zeroCopyCalls = take(gHpZeroCopy);
  stats->registeredHits = take(gHpRegHits);
  stats->pointerQueries = take(gHpQueries);
  stats->classifyNs = take(gHpClassifyNs);
  stats->copyNs = take(gHpCopyNs);
  stats->launchNs = take(gHpLaunchNs);
  stats->waitNs = take(gHpWaitNs);
  return nexrSuccess;
}

// Restates hostToDevRedOp (reference src/enqueue.cc:2185-2278) for the built-in ops.
NEXR_API nexrResult_t nexrHostToDevRedOp(nexrDevRedOpFull* opFull, int op, int datatype, int nRanks) {
  if (opFull == nullptr) return nexrInvalidArgument;
  const int nbits = 8 * (int)typeSize(datatype);
  if (nbits <= 0) return nexrInvalidArgument;
  const uint64_t allBits = ~(uint64_t)0 >> (64 - nbits);
  const uint64_t signBit = allBits ^ (allBits >> 1);
  opFull->scalarArgIsPtr = false;
  opFull->proxyOp = op;
  opFull->scalarArg = 0;
  switch (op) {
    case nexrSum: opFull->op = nexrDevSum; break;
    case nexrProd: opFull->op = nexrDevProd; break;
    case nexrMin:
    case nexrMax:
      opFull->op = nexrDevMinMax;
      if (isSignedInt(datatype)) opFull->scalarArg ^= signBit;
      opFull->scalarArg ^= (op == nexrMax) ? allBits : 0;
      break;
    case nexrAvg: {
      if (nRanks < 1) return nexrInvalidArgument;
      uint64_t u64 = 0;
      switch (datatype) {
        case nexrInt8: case nexrInt32: case nexrInt64:
        case nexrUint8: case nexrUint32: case nexrUint64:
          opFull->op = nexrDevSumPostDiv;
          u64 = ((uint64_t)nRanks << 1) | (isSignedInt(datatype) ? 1u : 0u);
          break;
        case nexrFloat16:
          opFull->op = nexrDevPreMulSum;
          u64 = floatToHalfRne((float)(1.0 / nRanks));
          break;
        case nexrBfloat16:
          opFull->op = nexrDevPreMulSum;
          u64 = floatToBf16Rne((float)(1.0 / nRanks));
          break;
        case nexrFloat32: {
          opFull->op = nexrDevPreMulSum;
          float f = (float)(1.0 / nRanks);
          uint32_t b;
          memcpy(&b, &f, 4);
          u64 = b;
          break;
        }
        case nexrFloat64: {
          opFull->op = nexrDevPreMulSum;
          double f = 1.0 / nRanks;
          memcpy(&u64, &f, 8);
          break;
        }
        default:  // fp8: the fork compiles this case out (enqueue.cc:2229-2238 guard)
          return nexrInvalidArgument;
      }
      opFull->scalarArg = u64;
      break;
    }
    default:  // user-created ops need a communicator's op table: not part of this boundary
      return nexrInvalidArgument;
  }
  return nexrSuccess;
}

// Restates ncclLaunchOneRank (reference src/device/onerank.cc:48-83).
NEXR_API nexrResult_t nexrLaunchOneRank(void* dst, const void* src, size_t nElts, nexrDevRedOpFull redOp,
                                        int datatype, nexrStream_t stream) {
  const size_t esz = typeSize(datatype);
  if (esz == 0) return nexrInvalidArgument;
  hipStream_t s = (hipStream_t)stream;
  if (redOp.op != nexrDevPreMulSum) {
    if (dst != src && nElts > 0) NEXR_HIP(hipMemcpyAsync(dst, src, nElts * esz, hipMemcpyDeviceToDevice, s));
    return nexrSuccess;
  }
  if (datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2) return nexrInvalidArgument;
  const void* srcs[1] = {src};
  void* dsts[1] = {dst};
  uint64_t arg = redOp.scalarArg;
  const void* prePtr = redOp.scalarArgIsPtr ? (const void*)(uintptr_t)redOp.scalarArg : nullptr;
  return reduceCopyDevice(1, srcs, 1, dsts, nElts, datatype, nexrDevPreMulSum, arg, 1, &arg, prePtr,
                          /*postOp=*/1, s);
}

NEXR_API nexrResult_t nexrReduceCopyLL(const void* src, int srcIsInput, int nRecv, const void* const* recvLines,
                                       const uint32_t* recvFlags, void* dst, int nSend, void* const* sendLines,
                                       const uint32_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                       uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                       nexrStream_t stream) {
  if (nRecv < 0 || nRecv > NEXR_MAX_SRCS || nSend < 0 || nSend > NEXR_MAX_DSTS) return nexrInvalidArgument;
  if (!src && nRecv == 0) return nexrInvalidArgument;   // LLGenericOp needs SRC or RECV
  if (!dst && nSend == 0) return nexrInvalidArgument;   // ... and DST or SEND
  if (datatype < 0 || datatype >= nexrNumTypes || datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2)
    return nexrInvalidArgument;
  if (devRedOp < 0 || devRedOp >= nexrNumDevRedOps) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && !isInteger(datatype)) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && (redOpArg & 1) != 0 && typeSize(datatype) == 1) {  // as validate()
    uint32_t divisor = (uint32_t)(redOpArg >> 1);
    if (divisor == 0) divisor = 1;
    if ((int8_t)divisor == 0) return nexrInvalidArgument;
  }
  if ((nRecv && (!recvLines || !recvFlags)) || (nSend && (!sendLines || !sendFlags))) return nexrInvalidArgument;
  if (nElts == 0) return nexrSuccess;
  LLParams a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < nRecv; i++) {
    if (!recvLines[i] || ((uintptr_t)recvLines[i] & 15)) return nexrInvalidArgument;
    a.recv[i] = (const char*)recvLines[i];
    a.recvFlag[i] = recvFlags[i];
  }
  for (int i = 0; i < nSend; i++) {
    if (!sendLines[i] || ((uintptr_t)sendLines[i] & 15)) return nexrInvalidArgument;
    a.send[i] = (char*)sendLines[i];
    a.sendFlag[i] = sendFlags[i];
  }
  a.src = (const char*)src;
  a.dst = (char*)dst;
  a.nElts = nElts;
  a.redArg = redOpArg;
  a.status = status;
  a.timeoutTicks = (uint64_t)(timeoutUs ? timeoutUs : 1000000u) * 100u;  // s_memrealtime: 100 MHz
  a.nRecv = nRecv;
  a.nSend = nSend;
  a.srcIsInput = srcIsInput ? 1 : 0;
  a.postOp = postOp ? 1 : 0;
  llSemantics(&datatype, &devRedOp, &a.srcIsInput, &a.postOp, &a.firstWins);
  const uint64_t nLines = (nElts * typeSize(datatype) + 7) / 8;
  uint64_t grid = (nLines + kLLTileLines - 1) / kLLTileLines;
  if (grid > (1u << 20)) grid = 1u << 20;
  NEXR_HIP(launch_ll(datatype, a, devRedOp, (int)grid, (hipStream_t)stream));
  return nexrSuccess;
}

// The steps run as if one at a time: a launch's workgroups walk its steps independently, which is
// only the same when no step touches user bytes that an earlier step of the launch wrote (or, for a
// write, read) at another element position. The same range at the same position is handled by the
// same lanes in both steps, in order.
namespace {
struct UserRange {
  uintptr_t beg, end;
  bool write;
};
bool rangesConflict(const std::vector<UserRange>& seen, const UserRange& r) {
  for (const UserRange& q : seen) {
    if (!r.write && !q.write) continue;
    if (r.beg < q.end && q.beg < r.end && !(r.beg == q.beg && r.end == q.end)) return true;
  }
  return false;
}
}  // namespace

// A flag rule is valid for nSlots slots (include/nexr.h): flagMax 0 or a power of two, cleanMask != 0 and a
// multiple of nSlots (the reference's static_assert, prims_ll.h), and the cleaning period
// 2^(msb(cleanMask) + 1) within the flag period, so that every line is rewritten before its flag recurs.
static bool llRuleValid(const nexrLLFlagRule& r, uint32_t nSlots) {
  if (r.flagMax & (r.flagMax - 1)) return false;
  if (r.cleanMask == 0 || nSlots == 0 || r.cleanMask % nSlots) return false;
  const uint64_t cleanPeriod = 2ull << (31 - __builtin_clz(r.cleanMask));
  const uint64_t flagPeriod = r.flagMax ? (uint64_t)r.flagMax : 1ull << 32;
  return cleanPeriod <= flagPeriod;
}

NEXR_API nexrResult_t nexrReduceCopyLLSteps(const nexrLLConnSet* cs, const nexrLLStep* steps, int nSteps,
                                            int datatype, int devRedOp, uint64_t redOpArg, uint32_t* status,
                                            uint32_t timeoutUs, nexrStream_t stream) {
  return nexrReduceCopyLLStepsRule(cs, steps, nSteps, datatype, devRedOp, redOpArg, nullptr, status, timeoutUs,
                                   stream);
}

// The argument checks of a run of LL steps of one Primitives (nexrReduceCopyLLStepsRule, and every member
// of nexrReduceCopyLLStepsGroup): nothing here touches the device. rule == nullptr: LL128 steps (every
// member of nexrReduceCopyLL128StepsGroup), whose slots are whole 2 KiB slices of 1920 data bytes and whose
// 64-bit flags need no rule.
static nexrResult_t llStepsValidate(const nexrLLConnSet* cs, const nexrLLStep* steps, int nSteps, int datatype,
                                    int devRedOp, uint64_t redOpArg, const nexrLLFlagRule* rule) {
  if (!cs || nSteps < 0 || (nSteps > 0 && !steps)) return nexrInvalidArgument;
  if (cs->nRecv < 0 || cs->nRecv > NEXR_LL_STEPS_MAX_PEERS || cs->nSend < 0 || cs->nSend > NEXR_LL_STEPS_MAX_PEERS)
    return nexrInvalidArgument;
  if (cs->slotBytes == 0 || cs->slotBytes % (rule ? 16 : kLL128SliceBytes) || cs->nSlots == 0) return nexrInvalidArgument;
  if (cs->nSlots > (uint32_t)INT_MAX) return nexrInvalidArgument;  // the kernels keep it as an int
  if (rule && !llRuleValid(*rule, cs->nSlots)) return nexrInvalidArgument;
  if (datatype < 0 || datatype >= nexrNumTypes || datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2)
    return nexrInvalidArgument;
  if (devRedOp < 0 || devRedOp >= nexrNumDevRedOps) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && !isInteger(datatype)) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && (redOpArg & 1) != 0 && typeSize(datatype) == 1) {  // as validate()
    uint32_t divisor = (uint32_t)(redOpArg >> 1);
    if (divisor == 0) divisor = 1;
    if ((int8_t)divisor == 0) return nexrInvalidArgument;
  }
  for (int i = 0; i < cs->nRecv; i++)
    if (!cs->recvFifo[i] || ((uintptr_t)cs->recvFifo[i] & 15) || !cs->recvHead[i] || ((uintptr_t)cs->recvHead[i] & 7))
      return nexrInvalidArgument;
  for (int i = 0; i < cs->nSend; i++)
    if (!cs->sendFifo[i] || ((uintptr_t)cs->sendFifo[i] & 15) || !cs->sendHead[i] || ((uintptr_t)cs->sendHead[i] & 7))
      return nexrInvalidArgument;
  const size_t esz = typeSize(datatype);
  // 8 data bytes per 16-byte line; LL128: 1920 per 2 KiB slice
  const uint64_t slotData = rule ? cs->slotBytes / 2 : cs->slotBytes / kLL128SliceBytes * kLL128SliceData;
  for (int k = 0; k < nSteps; k++) {
    const nexrLLStep& s = steps[k];
    if (s.srcBuf < -1 || s.srcBuf > 1 || s.dstBuf < -1 || s.dstBuf > 1) return nexrInvalidArgument;
    if ((s.recv && cs->nRecv == 0) || (s.send && cs->nSend == 0)) return nexrInvalidArgument;
    if ((s.srcBuf == 0 && !cs->input) || (s.srcBuf == 1 && !cs->output) || (s.dstBuf == 0 && !cs->input) ||
        (s.dstBuf == 1 && !cs->output))
      return nexrInvalidArgument;
    if (s.srcIx < 0 || s.dstIx < 0) return nexrInvalidArgument;
    if (s.nElts == 0) continue;
    if ((s.srcBuf < 0 && !s.recv) || (s.dstBuf < 0 && !s.send)) return nexrInvalidArgument;
    if ((s.recv || s.send) && (uint64_t)s.nElts * esz > slotData) return nexrInvalidArgument;
  }
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrReduceCopyLLStepsRule(const nexrLLConnSet* cs, const nexrLLStep* steps, int nSteps,
                                                int datatype, int devRedOp, uint64_t redOpArg,
                                                const nexrLLFlagRule* rulePtr, uint32_t* status, uint32_t timeoutUs,
                                                nexrStream_t stream) {
  const nexrLLFlagRule rule = rulePtr ? *rulePtr : nexrLLFlagRule{0u, 0x7ffffff8u};  // NULL: the production rule
  const nexrResult_t valid = llStepsValidate(cs, steps, nSteps, datatype, devRedOp, redOpArg, &rule);
  if (valid != nexrSuccess) return valid;
  if (nSteps == 0) return nexrSuccess;
  const size_t esz = typeSize(datatype);
  int srcIsInput = 1, postOp = 1;
  LLStepsParams P;
  memset(&P, 0, sizeof(P));
  llSemantics(&datatype, &devRedOp, &srcIsInput, &postOp, &P.firstWins);
  P.input = (const char*)cs->input;
  P.output = (char*)cs->output;
  for (int i = 0; i < NEXR_LL_STEPS_MAX_PEERS; i++) {
    P.recvFifo[i] = (const char*)cs->recvFifo[i];
    P.recvHead[i] = cs->recvHead[i];
    P.sendFifo[i] = (char*)cs->sendFifo[i];
    P.sendHead[i] = cs->sendHead[i];
  }
  P.slotBytes = cs->slotBytes;
  P.redArg = redOpArg;
  P.status = status;
  P.timeoutTicks = (uint64_t)(timeoutUs ? timeoutUs : 1000000u) * 100u;
  P.nRecv = cs->nRecv;
  P.nSend = cs->nSend;
  P.nSlots = (int)cs->nSlots;
  P.flagMask = rule.flagMax ? rule.flagMax - 1 : 0xffffffffu;
  // One workgroup per line tile of a full slot (the same grid on both ends of every connection).
  const uint64_t slotTiles = (cs->slotBytes / 16 + kLLTileLines - 1) / kLLTileLines;
  const int grid = (int)(slotTiles < 1 ? 1 : slotTiles > (uint64_t)kLLStepsMaxGrid ? kLLStepsMaxGrid : slotTiles);
  uint64_t rs[NEXR_LL_STEPS_MAX_PEERS], ss[NEXR_LL_STEPS_MAX_PEERS];
  for (int i = 0; i < NEXR_LL_STEPS_MAX_PEERS; i++) rs[i] = cs->recvStep[i], ss[i] = cs->sendStep[i];
  std::vector<UserRange> seen;
  auto launch = [&]() -> nexrResult_t {
    if (P.nSteps == 0) return nexrSuccess;
    NEXR_HIP(launch_ll_steps(datatype, P, devRedOp, grid, (hipStream_t)stream));
    P.nSteps = 0;
    seen.clear();
    return nexrSuccess;
  };
  for (int k = 0; k < nSteps; k++) {
    const nexrLLStep& s = steps[k];
    UserRange rd{0, 0, false}, wr{0, 0, true};
    if (s.nElts && s.srcBuf >= 0) {
      rd.beg = (uintptr_t)(s.srcBuf == 0 ? cs->input : cs->output) + (uintptr_t)s.srcIx * esz;
      rd.end = rd.beg + (uintptr_t)s.nElts * esz;
    }
    if (s.nElts && s.dstBuf >= 0) {
      wr.beg = (uintptr_t)(s.dstBuf == 0 ? cs->input : cs->output) + (uintptr_t)s.dstIx * esz;
      wr.end = wr.beg + (uintptr_t)s.nElts * esz;
    }
    if (P.nSteps == kLLStepsMax || (rd.end && rangesConflict(seen, rd)) || (wr.end && rangesConflict(seen, wr))) {
      nexrResult_t r = launch();
      if (r != nexrSuccess) return r;
    }
    if (P.nSteps == 0)
      for (int i = 0; i < NEXR_LL_STEPS_MAX_PEERS; i++) P.recvStep[i] = rs[i], P.sendStep[i] = ss[i];
    P.step[P.nSteps++] = s;
    if (rd.end) seen.push_back(rd);
    if (wr.end) seen.push_back(wr);
    // incSend's cleanup (prims_ll.h:85-93): a send step whose counter has every bit of the mask set cleans
    // its slot, per send connection. The launch ends at such a step and its kernel cleans after its last
    // step (nexr_ll.hip), so the step loop itself carries nothing for it.
    uint32_t cleans = 0;
    if (s.send)
      for (int j = 0; j < cs->nSend; j++)
        if (((uint32_t)ss[j] & rule.cleanMask) == rule.cleanMask) {
          cleans |= 1u << j;
          P.cleanStep[j] = ss[j];
        }
    if (s.recv)
      for (uint64_t& v : rs) v++;
    if (s.send)
      for (uint64_t& v : ss) v++;
    if (cleans) {
      P.cleanLast = cleans;
      nexrResult_t r = launch();
      P.cleanLast = 0;
      if (r != nexrSuccess) return r;
    }
  }
  return launch();
}

// ---- nexrReduceCopyLLStepsGroup: the runs of several Primitives in one launch ------------------------
// Three things make a group launch finish: its grid is resident as a whole (the occupancy
// check below), it needs nothing a later launch would produce (the dry run), and every poll of its
// kernel is bounded (nexr_ll.hip).
NEXR_API nexrResult_t nexrLLGroupWorkspaceBytes(int nMembers, size_t* bytes) {
  if (!bytes || nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS) return nexrInvalidArgument;
  *bytes = (size_t)nMembers * kLLGroupEntryBytes * NEXR_LL_GROUP_LAUNCHES;
  return nexrSuccess;
}

namespace {
// Workgroups of the group kernel the current device keeps resident (blocks per CU x CUs), looked up once
// per (device, datatype, op).
// Test hook: NEXR_TEST_LL_GROUP_RESIDENT=k makes the next calls take k as that number, so that the
// rejection of a grid that does not fit (and the ring's fall-back) can be tested on a GPU that fits it.
// Read per call (tests set it between calls).
nexrResult_t llGroupResident(bool ll128, int dt, int op, int64_t* resident) {
  if (const char* e = getenv("NEXR_TEST_LL_GROUP_RESIDENT"))
    if (*e) {
      *resident = strtoll(e, nullptr, 10);
      return nexrSuccess;
    }
  constexpr int kDevs = 16;
  static std::atomic<int64_t> cache[2][kDevs][nexrNumTypes][nexrNumDevRedOps];  // [LL, LL128]: a kernel each
  int dev = 0;
  NEXR_HIP(hipGetDevice(&dev));
  const bool cached = dev >= 0 && dev < kDevs;
  if (cached) {
    const int64_t v = cache[ll128][dev][dt][op].load(std::memory_order_relaxed);
    if (v > 0) {
      *resident = v;
      return nexrSuccess;
    }
  }
  int cus = 0, blocks = 0;
  NEXR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  NEXR_HIP(ll128 ? ll128_group_blocks_per_cu(dt, op, &blocks) : ll_group_blocks_per_cu(dt, op, &blocks));
  *resident = (int64_t)blocks * cus;
  if (cached && *resident > 0) cache[ll128][dev][dt][op].store(*resident, std::memory_order_relaxed);
  return nexrSuccess;
}

// The planner of the group calls (LL, LL128 and SIMPLE step lists), from the members' parameter blocks `cur`
// as they stand at the call's counters with no steps yet: the launch cuts, the dry run, the workspace and
// residency checks, the one copy of the tables and the launches. A recv / send step advances a
// connection's counters by `adv` (1, or SIMPLE's stepPerSlice) and a slot is free again nSlots steps later.
// rule: the LL flag rule, whose cleaning steps end a launch (nullptr: none).
extern "C++" {
// directRd(member, record): a further user range the record reads (a SIMPLE direct receive reads the member's
// output at dstIx), end == 0 for none.
template <typename Params, typename ResidentFn, typename LaunchFn, typename DirectRdFn>
nexrResult_t stepsGroupPlan(int nMembers, std::vector<Params>& cur, const nexrLLStep* const* steps, const int* nSteps,
                            int maxSteps, size_t esz, uint64_t adv, uint64_t nSlots, const nexrLLFlagRule* rule, int G,
                            ResidentFn residentFn, LaunchFn launchFn, DirectRdFn directRd, void* workspace,
                            size_t workspaceBytes, nexrStream_t stream) {
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  std::vector<Params> table;
  std::vector<std::vector<UserRange>> seen((size_t)nMembers);
  auto cut = [&]() {  // the launch is complete: its blocks go into the table, the next one starts at the counters
    for (int m = 0; m < nMembers; m++) {
      Params& P = cur[(size_t)m];
      table.push_back(P);
      for (int k = 0; k < P.nSteps; k++) {
        const nexrLLStep& s = P.step[k];
        for (int i = 0; i < MP; i++) P.recvStep[i] += s.recv ? adv : 0, P.sendStep[i] += s.send ? adv : 0;
      }
      P.nSteps = 0;
      if constexpr (std::is_same<Params, LLStepsParams>::value) P.cleanLast = 0;
      seen[(size_t)m].clear();
    }
  };
  int inLaunch = 0;  // step indices in the current launch
  for (int k = 0; k < maxSteps; k++) {
    bool before = inLaunch == kLLStepsMax, cleans = false;
    std::vector<UserRange> rd((size_t)nMembers, UserRange{0, 0, false}), wr((size_t)nMembers, UserRange{0, 0, true});
    std::vector<UserRange> rd2((size_t)nMembers, UserRange{0, 0, false});
    for (int m = 0; m < nMembers; m++) {
      if (k >= nSteps[m]) continue;
      const nexrLLStep& s = steps[m][k];
      const Params& cs = cur[(size_t)m];
      rd2[(size_t)m] = directRd(m, s);
      if (s.nElts && s.srcBuf >= 0) {
        rd[(size_t)m].beg = (uintptr_t)(s.srcBuf == 0 ? cs.input : cs.output) + (uintptr_t)s.srcIx * esz;
        rd[(size_t)m].end = rd[(size_t)m].beg + (uintptr_t)s.nElts * esz;
      }
      if (s.nElts && s.dstBuf >= 0) {
        wr[(size_t)m].beg = (uintptr_t)(s.dstBuf == 0 ? cs.input : cs.output) + (uintptr_t)s.dstIx * esz;
        wr[(size_t)m].end = wr[(size_t)m].beg + (uintptr_t)s.nElts * esz;
      }
      before = before || (rd[(size_t)m].end && rangesConflict(seen[(size_t)m], rd[(size_t)m])) ||
               (rd2[(size_t)m].end && rangesConflict(seen[(size_t)m], rd2[(size_t)m])) ||
               (wr[(size_t)m].end && rangesConflict(seen[(size_t)m], wr[(size_t)m]));
    }
    if (before && inLaunch) {
      cut();
      inLaunch = 0;
    }
    for (int m = 0; m < nMembers; m++) {
      if (k >= nSteps[m]) continue;
      const nexrLLStep& s = steps[m][k];
      Params& P = cur[(size_t)m];
      // the member's send counters at this step: those of the launch's start plus its send steps so far
      uint64_t sent = 0;
      for (int q = 0; q < P.nSteps; q++) sent += P.step[q].send ? 1 : 0;
      P.step[P.nSteps++] = s;
      if (rd[(size_t)m].end) seen[(size_t)m].push_back(rd[(size_t)m]);
      if (rd2[(size_t)m].end) seen[(size_t)m].push_back(rd2[(size_t)m]);
      if (wr[(size_t)m].end) seen[(size_t)m].push_back(wr[(size_t)m]);
      if constexpr (std::is_same<Params, LLStepsParams>::value) {
        if (s.send && rule)
          for (int j = 0; j < P.nSend; j++) {
            const uint64_t ss = P.sendStep[j] + sent;
            if (((uint32_t)ss & rule->cleanMask) == rule->cleanMask) {
              P.cleanLast |= 1u << j;
              P.cleanStep[j] = ss;
              cleans = true;
            }
          }
      }
    }
    inLaunch++;
    if (cleans) {
      cut();
      inLaunch = 0;
    }
  }
  if (inLaunch) cut();
  const size_t nLaunches = table.size() / (size_t)nMembers;

  // The dry run: every launch must finish with what it and the launches before it produce, because the
  // next one starts only behind it on the stream. Connections whose FIFO is some member's send FIFO and
  // another's receive FIFO are internal: their data and credit counters are walked here; the others are
  // taken as always ready (their peer runs elsewhere).
  struct Link {
    uint64_t sent, read;
  };
  std::vector<Link> links;
  std::vector<int> sendLink((size_t)nMembers * MP, -1), recvLink((size_t)nMembers * MP, -1);
  const Params* first = table.data();  // the first launch's blocks: the connections at the call's counters
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
    const Params* L = &table[l * (size_t)nMembers];
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

  // One region of the workspace per launch: a table is never written while a queued launch may read it.
  if (workspaceBytes / sizeof(Params) / (size_t)nMembers < nLaunches) return nexrInvalidArgument;

  // Co-residency: all nMembers * G workgroups at once, or a poll could wait for a workgroup that has no CU.
  int64_t resident = 0;
  const nexrResult_t occ = residentFn(&resident);
  if (occ != nexrSuccess) return occ;
  if ((int64_t)nMembers * G > resident) return nexrInvalidUsage;

  // Pageable source: the runtime has staged it when the call returns, so `table` may go out of scope.
  NEXR_HIP(hipMemcpyAsync(workspace, table.data(), table.size() * sizeof(Params), hipMemcpyHostToDevice,
                          (hipStream_t)stream));
  for (size_t l = 0; l < nLaunches; l++) NEXR_HIP(launchFn((const Params*)workspace + l * (size_t)nMembers));
  return nexrSuccess;
}
}  // extern "C++"

// The host side of both group calls: the argument checks, the launch cuts, the dry run, the workspace and
// residency checks, the one copy of the tables and the launches. rule == nullptr: LL128 steps
// (nexrReduceCopyLL128StepsGroup), which have no cleaning steps (so no cut behind one), slots counted in
// 2 KiB slices and a kernel (and so an occupancy) of their own; everything else is the same code.
nexrResult_t llStepsGroup(int nMembers, const nexrLLConnSet* conns, const nexrLLStep* const* steps, const int* nSteps,
                          int datatype, int devRedOp, uint64_t redOpArg, const nexrLLFlagRule* rule, uint32_t* status,
                          uint32_t timeoutUs, void* workspace, size_t workspaceBytes, nexrStream_t stream) {
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
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
  const uint64_t nSlots = conns[0].nSlots;
  int srcIsInput = 1, postOp = 1, firstWins = 0;
  llSemantics(&datatype, &devRedOp, &srcIsInput, &postOp, &firstWins);

  // The launches. A cut applies to every member at the same step index: before a step that would be a
  // member's 97th of the launch or that conflicts with user bytes the member touched earlier in it
  // (rangesConflict), and behind a step that cleans on any member (the kernel cleans behind a member's
  // last step). Entry (launch l, member m) of the table is that member's parameter block of launch l.
  std::vector<LLStepsParams> cur((size_t)nMembers);
  for (int m = 0; m < nMembers; m++) {
    const nexrLLConnSet& cs = conns[m];
    LLStepsParams& P = cur[(size_t)m];
    memset(&P, 0, sizeof(P));
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
    P.timeoutTicks = (uint64_t)(timeoutUs ? timeoutUs : 1000000u) * 100u;
    P.nRecv = cs.nRecv;
    P.nSend = cs.nSend;
    P.nSlots = (int)cs.nSlots;
    P.firstWins = firstWins;
    P.flagMask = rule && rule->flagMax ? rule->flagMax - 1 : 0xffffffffu;
  }
  // (a workgroup per tile of a slot: kLLTileLines 16-byte lines, or kLL128TileUnits 16-byte wire units)
  const uint64_t tileUnits = ll128 ? kLL128TileUnits : kLLTileLines;
  const uint64_t slotTiles = (conns[0].slotBytes / 16 + tileUnits - 1) / tileUnits;
  const int G = (int)(slotTiles < 1 ? 1 : slotTiles > (uint64_t)kLLStepsMaxGrid ? kLLStepsMaxGrid : slotTiles);
  return stepsGroupPlan(
      nMembers, cur, steps, nSteps, maxSteps, esz, 1, nSlots, rule, G,
      [&](int64_t* resident) { return llGroupResident(ll128, datatype, devRedOp, resident); },
      [&](const LLStepsParams* entries) {
        return ll128 ? launch_ll128_group(datatype, devRedOp, entries, nMembers, G, (hipStream_t)stream)
                     : launch_ll_group(datatype, devRedOp, entries, nMembers, G, (hipStream_t)stream);
      },
      [](int, const nexrLLStep&) { return UserRange{0, 0, false}; }, workspace, workspaceBytes, stream);
}
}  // namespace

NEXR_API nexrResult_t nexrReduceCopyLLStepsGroup(int nMembers, const nexrLLConnSet* conns,
                                                 const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                 int devRedOp, uint64_t redOpArg, const nexrLLFlagRule* rulePtr,
                                                 uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                 size_t workspaceBytes, nexrStream_t stream) {
  const nexrLLFlagRule rule = rulePtr ? *rulePtr : nexrLLFlagRule{0u, 0x7ffffff8u};  // NULL: the production rule
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

// ---- nexrReduceCopySimpleStepsGroup: SIMPLE step lists of several Primitives in one launch ------------
NEXR_API nexrResult_t nexrSimpleGroupWorkspaceBytes(int nMembers, size_t* bytes) {
  if (!bytes || nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS) return nexrInvalidArgument;
  *bytes = (size_t)nMembers * sizeof(SimpleStepsParams) * NEXR_LL_GROUP_LAUNCHES;
  return nexrSuccess;
}

namespace {
// Workgroups of the SIMPLE group kernel the current device keeps resident, as llGroupResident. The
// hardware admits 256-thread workgroups by their scalar registers too, and for kernels that use more than
// 80 of them one fewer per CU than the occupancy query says; a surplus workgroup would queue until a
// resident one exits, which a poll may be waiting for. So one is taken off the query's answer.
// Test hook: NEXR_TEST_SIMPLE_GROUP_RESIDENT=k makes the next calls take k as that number (read per call).
// direct: the kernel variant of nexrReduceCopySimpleStepsGroupDirect (the one that is launched is queried).
nexrResult_t simpleGroupResident(bool direct, int dt, int op, int64_t* resident) {
  if (const char* e = getenv("NEXR_TEST_SIMPLE_GROUP_RESIDENT"))
    if (*e) {
      *resident = strtoll(e, nullptr, 10);
      return nexrSuccess;
    }
  constexpr int kDevs = 16;
  static std::atomic<int64_t> cache[2][kDevs][nexrNumTypes][nexrNumDevRedOps];  // [FIFO-only, direct]
  int dev = 0;
  NEXR_HIP(hipGetDevice(&dev));
  const bool cached = dev >= 0 && dev < kDevs;
  if (cached) {
    const int64_t v = cache[direct][dev][dt][op].load(std::memory_order_relaxed);
    if (v > 0) {
      *resident = v;
      return nexrSuccess;
    }
  }
  int cus = 0, blocks = 0;
  NEXR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  NEXR_HIP(direct ? simple_group_direct_blocks_per_cu(dt, op, &blocks) : simple_group_blocks_per_cu(dt, op, &blocks));
  if (blocks > 8) blocks = 8;
  if (blocks > 1) blocks--;
  *resident = (int64_t)blocks * cus;
  if (cached && *resident > 0) cache[direct][dev][dt][op].store(*resident, std::memory_order_relaxed);
  return nexrSuccess;
}

// The host side of both SIMPLE group calls. direct == nullptr: nexrReduceCopySimpleStepsGroup, the FIFO-only
// kernels and their table entry; else one nexrSimpleDirectSet per member, the direct kernels and theirs.
nexrResult_t simpleStepsGroup(int nMembers, const nexrSimpleConnSet* conns, const nexrLLStep* const* steps,
                              const int* nSteps, int datatype, int devRedOp, uint64_t redOpArg,
                              int workgroupsPerMember, const nexrSimpleDirectSet* direct, uint32_t* status,
                              uint32_t timeoutUs, void* workspace, size_t workspaceBytes, nexrStream_t stream) {
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  if (nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS || !conns || !steps || !nSteps) return nexrInvalidArgument;
  if (workgroupsPerMember < 0 || workgroupsPerMember > NEXR_SIMPLE_GROUP_MAX_GRID) return nexrInvalidArgument;
  if (datatype < 0 || datatype >= nexrNumTypes || datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2)
    return nexrInvalidArgument;
  if (devRedOp < 0 || devRedOp >= nexrNumDevRedOps) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && !isInteger(datatype)) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && (redOpArg & 1) != 0 && typeSize(datatype) == 1) {  // as validate()
    uint32_t divisor = (uint32_t)(redOpArg >> 1);
    if (divisor == 0) divisor = 1;
    if ((int8_t)divisor == 0) return nexrInvalidArgument;
  }
  const size_t esz = typeSize(datatype);
  int maxSteps = 0;
  for (int m = 0; m < nMembers; m++) {
    const nexrSimpleConnSet& cs = conns[m];
    if (nSteps[m] < 0 || (nSteps[m] > 0 && !steps[m])) return nexrInvalidArgument;
    if (cs.nRecv < 0 || cs.nRecv > MP || cs.nSend < 0 || cs.nSend > MP) return nexrInvalidArgument;
    if (cs.slotBytes == 0 || cs.slotBytes % 16 || cs.nSlots == 0 || cs.nSlots > (uint32_t)INT_MAX)
      return nexrInvalidArgument;
    if (cs.stepPerSlice < 1 || cs.nSlots % cs.stepPerSlice) return nexrInvalidArgument;
    // one G, one credit window and one slice size serve the launch
    if (cs.slotBytes != conns[0].slotBytes || cs.nSlots != conns[0].nSlots || cs.stepPerSlice != conns[0].stepPerSlice)
      return nexrInvalidArgument;
    for (int i = 0; i < cs.nRecv; i++)
      if (!cs.recvFifo[i] || ((uintptr_t)cs.recvFifo[i] & 15) || !cs.recvTail[i] || ((uintptr_t)cs.recvTail[i] & 7) ||
          !cs.recvHead[i] || ((uintptr_t)cs.recvHead[i] & 7) || cs.recvStep[i] % cs.stepPerSlice)
        return nexrInvalidArgument;
    for (int i = 0; i < cs.nSend; i++)
      if (!cs.sendFifo[i] || ((uintptr_t)cs.sendFifo[i] & 15) || !cs.sendTail[i] || ((uintptr_t)cs.sendTail[i] & 7) ||
          !cs.sendHead[i] || ((uintptr_t)cs.sendHead[i] & 7) || cs.sendStep[i] % cs.stepPerSlice)
        return nexrInvalidArgument;
    const uint64_t sliceBytes = cs.slotBytes * cs.stepPerSlice;
    for (int k = 0; k < nSteps[m]; k++) {
      const nexrLLStep& s = steps[m][k];
      if (s.srcBuf < -1 || s.srcBuf > 1 || s.dstBuf < -1 || s.dstBuf > 1) return nexrInvalidArgument;
      if ((s.recv && cs.nRecv == 0) || (s.send && cs.nSend == 0)) return nexrInvalidArgument;
      if ((s.srcBuf == 0 && !cs.input) || (s.srcBuf == 1 && !cs.output) || (s.dstBuf == 0 && !cs.input) ||
          (s.dstBuf == 1 && !cs.output))
        return nexrInvalidArgument;
      if (s.srcIx < 0 || s.dstIx < 0) return nexrInvalidArgument;
      if (s.nElts == 0) continue;
      if ((s.srcBuf < 0 && !s.recv) || (s.dstBuf < 0 && !s.send)) return nexrInvalidArgument;
      if ((uint64_t)s.nElts * esz > sliceBytes) return nexrInvalidArgument;
    }
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
  auto fill = [&](SimpleStepsParams& P, const nexrSimpleConnSet& cs) {
    P.input = (const char*)cs.input;
    P.output = (char*)cs.output;
    for (int i = 0; i < MP; i++) {
      P.recvFifo[i] = (const char*)cs.recvFifo[i];
      P.recvTail[i] = cs.recvTail[i];
      P.recvHead[i] = cs.recvHead[i];
      P.sendFifo[i] = (char*)cs.sendFifo[i];
      P.sendTail[i] = cs.sendTail[i];
      P.sendHead[i] = cs.sendHead[i];
      P.recvStep[i] = cs.recvStep[i];
      P.sendStep[i] = cs.sendStep[i];
    }
    P.slotBytes = cs.slotBytes;
    P.redArg = redOpArg;
    P.status = status;
    P.timeoutTicks = (uint64_t)(timeoutUs ? timeoutUs : 1000000u) * 100u;
    P.nRecv = cs.nRecv;
    P.nSend = cs.nSend;
    P.nSlots = (int)cs.nSlots;
    P.firstWins = firstWins;
    P.stepPerSlice = (int)cs.stepPerSlice;
  };
  if (direct) {
    std::vector<SimpleDirectParams> cur((size_t)nMembers);
    for (int m = 0; m < nMembers; m++) {
      SimpleDirectParams& P = cur[(size_t)m];
      memset((void*)&P, 0, sizeof(P));
      fill(P, conns[m]);
      for (int j = 0; j < conns[m].nSend; j++) P.sendDirect[j] = (char*)direct[m].sendDirect[j];
      P.recvDirect = direct[m].recvDirect[0] ? 1 : 0;
    }
    return stepsGroupPlan(
        nMembers, cur, steps, nSteps, maxSteps, esz, sps, conns[0].nSlots, nullptr, G,
        [&](int64_t* resident) { return simpleGroupResident(true, datatype, devRedOp, resident); },
        [&](const SimpleDirectParams* entries) {
          return launch_simple_group_direct(datatype, devRedOp, entries, nMembers, G, (hipStream_t)stream);
        },
        [&](int m, const nexrLLStep& st) {  // a direct source: the member's output at dstIx
          UserRange rd{0, 0, false};
          if (st.nElts && st.recv && (st.pad[0] & NEXR_SIMPLE_DIRECT_RECV) && direct[m].recvDirect[0]) {
            rd.beg = (uintptr_t)conns[m].output + (uintptr_t)st.dstIx * esz;
            rd.end = rd.beg + (uintptr_t)st.nElts * esz;
          }
          return rd;
        },
        workspace, workspaceBytes, stream);
  }
  std::vector<SimpleStepsParams> cur((size_t)nMembers);
  for (int m = 0; m < nMembers; m++) {
    memset(&cur[(size_t)m], 0, sizeof(SimpleStepsParams));
    fill(cur[(size_t)m], conns[m]);
  }
  return stepsGroupPlan(
      nMembers, cur, steps, nSteps, maxSteps, esz, sps, conns[0].nSlots, nullptr, G,
      [&](int64_t* resident) { return simpleGroupResident(false, datatype, devRedOp, resident); },
      [&](const SimpleStepsParams* entries) {
        return launch_simple_group(datatype, devRedOp, entries, nMembers, G, (hipStream_t)stream);
      },
      [](int, const nexrLLStep&) { return UserRange{0, 0, false}; }, workspace, workspaceBytes, stream);
}
}  // namespace

NEXR_API nexrResult_t nexrReduceCopySimpleStepsGroup(int nMembers, const nexrSimpleConnSet* conns,
                                                     const nexrLLStep* const* steps, const int* nSteps, int datatype,
                                                     int devRedOp, uint64_t redOpArg, int workgroupsPerMember,
                                                     uint32_t* status, uint32_t timeoutUs, void* workspace,
                                                     size_t workspaceBytes, nexrStream_t stream) {
  return simpleStepsGroup(nMembers, conns, steps, nSteps, datatype, devRedOp, redOpArg, workgroupsPerMember, nullptr,
                          status, timeoutUs, workspace, workspaceBytes, stream);
}

NEXR_API nexrResult_t nexrSimpleGroupDirectWorkspaceBytes(int nMembers, size_t* bytes) {
  if (!bytes || nMembers < 1 || nMembers > NEXR_LL_GROUP_MAX_MEMBERS) return nexrInvalidArgument;
  *bytes = (size_t)nMembers * sizeof(SimpleDirectParams) * NEXR_LL_GROUP_LAUNCHES;
  return nexrSuccess;
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
  if (!inputs || !outputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS || nBlocks < 0 || nBlocks > 64) return nexrInvalidArgument;
  if (datatype != nexrFloat32 && datatype != nexrFloat16 && datatype != nexrBfloat16) return nexrInvalidArgument;
  if (devRedOp != nexrDevSum) return nexrInvalidArgument;
  const uint64_t esz = typeSize(datatype);
  SymParams p;
  memset(&p, 0, sizeof(p));
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || !outputs[r]) return nexrInvalidArgument;
    if (((uintptr_t)inputs[r] | (uintptr_t)outputs[r]) & (esz - 1)) return nexrInvalidArgument;
    p.in[r] = (const char*)inputs[r];
    p.out[r] = (char*)outputs[r];
  }
  if (nElts > (size_t)-1 / esz) return nexrInvalidArgument;
  if (nElts == 0) return nexrSuccess;
  symPlan((uintptr_t)inputs[0], (uintptr_t)outputs[0], nElts, esz, (uint64_t)nRanks * (uint64_t)(nBlocks ? nBlocks : 1),
          &p);
  p.nRanks = nRanks;
  p.nFold = semantics() == nexrSemanticsShipped ? 1 : nRanks;  // SKIP_COMP: every add returns its first operand
  // One-shot: a wave per piece or group of 32 end elements, four waves per workgroup; beyond the cap the
  // kernel strides.
  const uint64_t items = p.p1Pieces + p.p2Pieces + (p.nEnds + 31) / 32;
  const uint64_t grid = std::min<uint64_t>((items + kBlock / 64 - 1) / (kBlock / 64), gridCap(kBlock));
  NEXR_HIP(launch_sym_all_reduce(datatype, p, (unsigned)grid, (hipStream_t)stream));
  return nexrSuccess;
}

// The one-shot grid of the symmetric reduce-scatter and all-gather: every chunk of chunkBytes is whole
// 2048-byte pieces, groups of 64 16-byte packs and one tail item; a wave per item and rank, four waves per
// workgroup; beyond the cap the kernels stride.
static unsigned symChunkGrid(uint64_t chunkBytes, uint64_t esz, int nRanks) {
  const uint64_t rem = chunkBytes % 2048;
  const uint64_t perRank = chunkBytes / 2048 + (rem / 16 + 63) / 64 + (rem % 16 / esz ? 1 : 0);
  const uint64_t items = perRank * (uint64_t)nRanks;
  return (unsigned)std::min<uint64_t>((items + kBlock / 64 - 1) / (kBlock / 64), gridCap(kBlock));
}

NEXR_API nexrResult_t nexrSymReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                           size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                           nexrStream_t stream) {
  (void)redOpArg;
  if (!inputs || !outputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  if (datatype != nexrFloat32 && datatype != nexrFloat16 && datatype != nexrBfloat16) return nexrInvalidArgument;
  if (devRedOp != nexrDevSum) return nexrInvalidArgument;
  const uint64_t esz = typeSize(datatype);
  SymRsParams p;
  memset(&p, 0, sizeof(p));
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || !outputs[r]) return nexrInvalidArgument;
    if (((uintptr_t)inputs[r] | (uintptr_t)outputs[r]) & (esz - 1)) return nexrInvalidArgument;
    p.in[r] = (const char*)inputs[r];
    p.out[r] = (char*)outputs[r];
  }
  if (nElts > (size_t)-1 / esz / (size_t)nRanks) return nexrInvalidArgument;  // an input's nRanks * nElts * esz bytes
  if (nElts == 0) return nexrSuccess;
  p.chunkBytes = (uint64_t)nElts * esz;
  p.nRanks = nRanks;
  p.nFold = semantics() == nexrSemanticsShipped ? 1 : nRanks;  // SKIP_COMP: every add returns its first operand
  NEXR_HIP(launch_sym_reduce_scatter(datatype, p, symChunkGrid(p.chunkBytes, esz, nRanks), (hipStream_t)stream));
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrSymAllGather(int nRanks, const void* const* inputs, void* const* outputs, size_t nBytes,
                                       nexrStream_t stream) {
  if (!inputs || !outputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  if (nBytes > (size_t)-1 / (size_t)nRanks) return nexrInvalidArgument;  // an output's nRanks * nBytes bytes
  SymAgParams p;
  memset(&p, 0, sizeof(p));
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || !outputs[r]) return nexrInvalidArgument;
    p.in[r] = (const char*)inputs[r];
    p.out[r] = (char*)outputs[r];
    // the reference's inPlace, per rank
    if ((uintptr_t)inputs[r] == (uintptr_t)outputs[r] + (uintptr_t)r * nBytes) p.inPlace |= 1ull << r;
  }
  if (nBytes == 0) return nexrSuccess;
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
nexrResult_t flatPrepare(int nRanks, const void* const* inputs, int datatype, int devRedOp, uint64_t redOpArg,
                         int userFirst, FlatParams* p, int* dt, int* op) {
  if (!inputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  if (datatype < 0 || datatype >= nexrNumTypes || datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2)
    return nexrInvalidArgument;
  if (devRedOp < 0 || devRedOp >= nexrNumDevRedOps) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && !isInteger(datatype)) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && (redOpArg & 1) != 0 && typeSize(datatype) == 1) {  // as validate()
    uint32_t divisor = (uint32_t)(redOpArg >> 1);
    if (divisor == 0) divisor = 1;
    if ((int8_t)divisor == 0) return nexrInvalidArgument;
  }
  const uint64_t esz = typeSize(datatype);
  memset((void*)p, 0, sizeof(*p));
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || ((uintptr_t)inputs[r] & (esz - 1))) return nexrInvalidArgument;
    p->in[r] = (const char*)inputs[r];
  }
  int srcIsInput = 1, postOp = 1, firstWins = 0;
  *dt = datatype;
  *op = devRedOp;
  llSemantics(dt, op, &srcIsInput, &postOp, &firstWins);
  p->nRanks = nRanks;
  p->redArg = redOpArg;
  p->userFirst = userFirst ? 1 : 0;
  p->nFold = firstWins ? 1 : nRanks;
  p->shift = firstWins && userFirst ? nRanks - 1 : 0;
  p->preOp = srcIsInput;
  p->postOp = postOp;
  return nexrSuccess;
}

// One-shot: a wave per 2048-byte piece of every region, four waves per workgroup; beyond the cap the kernel
// strides.
unsigned flatGrid(uint64_t regionBytes, int nRegions, uint64_t maxGrid = 0) {
  const uint64_t items = (regionBytes + 2047) / 2048 * (uint64_t)nRegions;
  const uint64_t grid = std::min<uint64_t>((items + kBlock / 64 - 1) / (kBlock / 64), gridCap(kBlock));
  return (unsigned)(maxGrid > 0 && grid > maxGrid ? maxGrid : grid);  // maxGrid: the host forms' cap (hostGrid)
}
}  // namespace

// The checks of nexrFlatAllReduce, and the launch's parameters over the pointers as given (no device call).
namespace {
nexrResult_t flatAllReduceCheck(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                const nexrFlatPart* parts, int nParts, FlatParams* pp, int* dtp, int* opp) {
  FlatParams& p = *pp;
  int& dt = *dtp;
  int& op = *opp;
  if (!outputs) return nexrInvalidArgument;
  nexrResult_t res = flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess) return res;
  const uint64_t esz = typeSize(datatype), epp = 16 / esz;
  for (int r = 0; r < nRanks; r++) {
    if (!outputs[r] || ((uintptr_t)outputs[r] & (esz - 1))) return nexrInvalidArgument;
    p.out[r] = (char*)outputs[r];
  }
  if (nElts > (size_t)-1 / esz) return nexrInvalidArgument;
  if (nParts < 0 || (nParts > 0 && !parts)) return nexrInvalidArgument;
  uint64_t at = 0;
  for (int k = 0; k < nParts; k++) {  // ascending, gapless, from 0
    const nexrFlatPart& q = parts[k];
    if (q.offset != at || q.count == 0 || q.count > (uint64_t)nElts - at) return nexrInvalidArgument;
    if (q.offset % epp || q.chunkCount == 0 || q.chunkCount % epp) return nexrInvalidArgument;
    if (q.chunkCount > (uint64_t)-1 / (uint64_t)nRanks) return nexrInvalidArgument;
    at += q.count;
  }
  if (at != (uint64_t)nElts) return nexrInvalidArgument;
  p.coll = kFlatAllReduce;
  p.regionBytes = p.winEnd = (uint64_t)nElts * esz;
  p.nParts = nParts;
  p.nOut = nRanks;
  return nexrSuccess;
}

// A part list too long for a launch's arguments, in a stream-ordered workspace: the parts travel by value in
// short launches ahead of the one, so nothing is read after return. The caller frees *ws behind its launch.
nexrResult_t flatPartsWorkspace(const nexrFlatPart* parts, int nParts, hipStream_t s, nexrFlatPart** ws) {
  NEXR_HIP(hipMallocAsync((void**)ws, (size_t)nParts * sizeof(nexrFlatPart), s));
  FlatPartsFill f;
  for (int k = 0; k < nParts; k += kFlatInlineParts) {
    f.dst = *ws + k;
    f.n = std::min(kFlatInlineParts, nParts - k);
    f.pad = 0;
    memcpy(f.parts, parts + k, (size_t)f.n * sizeof(nexrFlatPart));
    const hipError_t e = launch_flat_parts(f, s);
    if (e != hipSuccess) {
      (void)hipFreeAsync(*ws, s);
      *ws = nullptr;
      return hipFail(e);
    }
  }
  return nexrSuccess;
}

// One launch of a checked all-reduce over the window that p holds; gridCap > 0 caps the grid.
nexrResult_t flatAllReduceLaunch(FlatParams& p, int dt, int op, const nexrFlatPart* parts, int nParts,
                                 uint64_t gridCapWgs, hipStream_t s) {
  nexrFlatPart* ws = nullptr;
  if (nParts <= kFlatInlineParts) {
    memcpy(p.parts, parts, (size_t)nParts * sizeof(nexrFlatPart));
  } else {
    const nexrResult_t res = flatPartsWorkspace(parts, nParts, s, &ws);
    if (res != nexrSuccess) return res;
    p.ext = ws;
  }
  const hipError_t e = launch_flat(dt, op, p, flatGrid(p.winEnd - p.winBeg, 1, gridCapWgs), s);
  if (ws) (void)hipFreeAsync(ws, s);
  NEXR_HIP(e);
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatAllReduce(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                        int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                        const nexrFlatPart* parts, int nParts, nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  const nexrResult_t res = flatAllReduceCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst,
                                              parts, nParts, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  return flatAllReduceLaunch(p, dt, op, parts, nParts, 0, (hipStream_t)stream);
}

namespace {
nexrResult_t flatReduceScatterCheck(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts,
                                    int datatype, int devRedOp, uint64_t redOpArg, int userFirst, FlatParams* pp,
                                    int* dtp, int* opp) {
  FlatParams& p = *pp;
  int& dt = *dtp;
  int& op = *opp;
  if (!outputs) return nexrInvalidArgument;
  nexrResult_t res = flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess) return res;
  const uint64_t esz = typeSize(datatype);
  for (int r = 0; r < nRanks; r++) {
    if (!outputs[r] || ((uintptr_t)outputs[r] & (esz - 1))) return nexrInvalidArgument;
    p.out[r] = (char*)outputs[r];
  }
  if (nElts > (size_t)-1 / esz / (size_t)nRanks) return nexrInvalidArgument;  // an input's nRanks * nElts * esz bytes
  p.coll = kFlatReduceScatter;
  p.regionBytes = p.winEnd = (uint64_t)nElts * esz;
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  const nexrResult_t res =
      flatReduceScatterCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  NEXR_HIP(launch_flat(dt, op, p, flatGrid(p.regionBytes, nRanks), (hipStream_t)stream));
  return nexrSuccess;
}

namespace {
nexrResult_t flatReduceCheck(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                             int datatype, int devRedOp, uint64_t redOpArg, int userFirst, FlatParams* pp, int* dtp,
                             int* opp) {
  FlatParams& p = *pp;
  int& dt = *dtp;
  int& op = *opp;
  if (!output) return nexrInvalidArgument;
  nexrResult_t res = flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess) return res;
  const uint64_t esz = typeSize(datatype);
  if (root < 0 || root >= nRanks || ((uintptr_t)output & (esz - 1))) return nexrInvalidArgument;
  if (nElts > (size_t)-1 / esz) return nexrInvalidArgument;
  p.out[root] = (char*)output;
  p.root = root;
  p.coll = kFlatReduce;
  p.regionBytes = p.winEnd = (uint64_t)nElts * esz;
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatReduce(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                                     int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                     nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  const nexrResult_t res =
      flatReduceCheck(nRanks, inputs, output, root, nElts, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  NEXR_HIP(launch_flat(dt, op, p, flatGrid(p.regionBytes, 1), (hipStream_t)stream));
  return nexrSuccess;
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
}  // namespace

namespace {
nexrResult_t flatTreeCheck(int nRanks, const void* const* inputs, void* const* outputs, size_t nElts, int datatype,
                           int devRedOp, uint64_t redOpArg, int userFirst, const nexrFlatTreeLinks* const* trees,
                           int nTrees, const nexrFlatTreePart* parts, int nParts, FlatTreeParams* pp, int* dtp,
                           int* opp) {
  FlatTreeParams& p = *pp;
  int& dt = *dtp;
  int& op = *opp;
  FlatParams fp;  // the shared checks and what the semantics make of the call
  if (!outputs) return nexrInvalidArgument;
  nexrResult_t res = flatPrepare(nRanks, inputs, datatype, devRedOp, redOpArg, userFirst, &fp, &dt, &op);
  if (res != nexrSuccess) return res;
  const uint64_t esz = typeSize(datatype), epp = 16 / esz;
  memset((void*)&p, 0, sizeof(p));
  for (int r = 0; r < nRanks; r++) {
    if (!outputs[r] || ((uintptr_t)outputs[r] & (esz - 1))) return nexrInvalidArgument;
    p.in[r] = fp.in[r];
    p.out[r] = (char*)outputs[r];
  }
  if (nElts > (size_t)-1 / esz) return nexrInvalidArgument;
  if (!trees || nTrees < 1 || nTrees > 2) return nexrInvalidArgument;
  if (nParts < 0 || (nParts > 0 && !parts)) return nexrInvalidArgument;
  const bool firstWins = fp.nFold == 1;
  for (int t = 0; t < nTrees; t++) {
    if (!trees[t]) return nexrInvalidArgument;
    std::vector<uint8_t> code;
    int need = 0, root = -1;
    if (!flatTreeCompile(trees[t], nRanks, &code, &need, &root)) return nexrInvalidArgument;
    if (need > kFlatTreeSlots || code.size() > (size_t)kFlatTreeProgBytes) return nexrInvalidArgument;
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
  uint64_t at = 0;
  for (int k = 0; k < nParts; k++) {  // ascending, gapless, from 0
    const nexrFlatTreePart& q = parts[k];
    if (q.offset != at || q.count == 0 || q.count > (uint64_t)nElts - at) return nexrInvalidArgument;
    if (q.offset % epp || q.tree >= (uint32_t)nTrees) return nexrInvalidArgument;
    at += q.count;
  }
  if (at != (uint64_t)nElts) return nexrInvalidArgument;
  p.nBytes = p.winEnd = (uint64_t)nElts * esz;
  p.redArg = fp.redArg;
  p.nRanks = p.nOut = nRanks;
  p.userFirst = fp.userFirst;
  p.preOp = fp.preOp;
  p.postOp = fp.postOp;
  p.nParts = nParts;
  return nexrSuccess;
}

// flatPartsWorkspace for a tree's parts.
nexrResult_t flatTreePartsWorkspace(const nexrFlatTreePart* parts, int nParts, hipStream_t s, nexrFlatTreePart** ws) {
  NEXR_HIP(hipMallocAsync((void**)ws, (size_t)nParts * sizeof(nexrFlatTreePart), s));
  FlatTreePartsFill f;
  for (int k = 0; k < nParts; k += kFlatTreeInlineParts) {
    f.dst = *ws + k;
    f.n = std::min(kFlatTreeInlineParts, nParts - k);
    f.pad = 0;
    memcpy(f.parts, parts + k, (size_t)f.n * sizeof(nexrFlatTreePart));
    const hipError_t e = launch_flat_tree_parts(f, s);
    if (e != hipSuccess) {
      (void)hipFreeAsync(*ws, s);
      *ws = nullptr;
      return hipFail(e);
    }
  }
  return nexrSuccess;
}

// One launch of a checked tree all-reduce over the window that p holds; gridCapWgs > 0 caps the grid.
nexrResult_t flatTreeLaunch(FlatTreeParams& p, int dt, int op, const nexrFlatTreePart* parts, int nParts,
                            uint64_t gridCapWgs, hipStream_t s) {
  nexrFlatTreePart* ws = nullptr;
  if (nParts <= kFlatTreeInlineParts) {
    memcpy(p.parts, parts, (size_t)nParts * sizeof(nexrFlatTreePart));
  } else {
    const nexrResult_t res = flatTreePartsWorkspace(parts, nParts, s, &ws);
    if (res != nexrSuccess) return res;
    p.ext = ws;
  }
  const hipError_t e = launch_flat_tree(dt, op, p, flatGrid(p.winEnd - p.winBeg, 1, gridCapWgs), s);
  if (ws) (void)hipFreeAsync(ws, s);
  NEXR_HIP(e);
  return nexrSuccess;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatTreeAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                            size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                            int userFirst, const nexrFlatTreeLinks* const* trees, int nTrees,
                                            const nexrFlatTreePart* parts, int nParts, nexrStream_t stream) {
  FlatTreeParams p;
  int dt, op;
  const nexrResult_t res = flatTreeCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst,
                                         trees, nTrees, parts, nParts, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  return flatTreeLaunch(p, dt, op, parts, nParts, 0, (hipStream_t)stream);
}

// ---- nexrFlat*PreMul: PreMulSum with a scalar per rank --------------------------------------------------------
// The plain entry's checks run with nexrDevPreMulSum and make the plain launch's parameters; the scalars are
// checked; then the fields move into the per-rank kernels' block. Under nexrSemanticsShipped the checks turn the
// op into a bit copy without a pre-op: that is the plain kernel's launch, and no scalar is read.
namespace {
nexrResult_t flatScalarsCheck(int nRanks, const uint64_t* scalars, int arePtrs, int datatype) {
  if (!scalars) return nexrInvalidArgument;
  const uint64_t esz = typeSize(datatype);
  for (int r = 0; arePtrs && r < nRanks; r++)
    if (!scalars[r] || (scalars[r] & (esz - 1))) return nexrInvalidArgument;
  return nexrSuccess;
}

void flatPreMulFrom(const FlatParams& p, const uint64_t* scalars, int arePtrs, FlatPreMulParams* q) {
  memset((void*)q, 0, sizeof(*q));
  memcpy(q->in, p.in, sizeof(q->in));
  memcpy(q->out, p.out, sizeof(q->out));
  memcpy(q->scalars, scalars, (size_t)p.nRanks * sizeof(uint64_t));
  q->regionBytes = p.regionBytes;
  q->winBeg = p.winBeg;
  q->winEnd = p.winEnd;
  q->coll = p.coll;
  q->nRanks = p.nRanks;
  q->nFold = p.nFold;
  q->shift = p.shift;
  q->userFirst = p.userFirst;
  q->preOp = p.preOp;
  q->postOp = p.postOp;
  q->root = p.root;
  q->nParts = p.nParts;
  q->nOut = p.nOut;
  q->scalarsArePtrs = arePtrs ? 1 : 0;
}
}  // namespace

NEXR_API nexrResult_t nexrFlatAllReducePreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                              size_t nElts, int datatype, const uint64_t* scalars,
                                              int scalarsArePtrs, int userFirst, const nexrFlatPart* parts,
                                              int nParts, nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  nexrResult_t res = flatAllReduceCheck(nRanks, inputs, outputs, nElts, datatype, nexrDevPreMulSum, 0, userFirst, parts,
                                        nParts, &p, &dt, &op);
  if (res == nexrSuccess) res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (res != nexrSuccess || nElts == 0) return res;
  hipStream_t s = (hipStream_t)stream;
  if (op != nexrDevPreMulSum) return flatAllReduceLaunch(p, dt, op, parts, nParts, 0, s);
  FlatPreMulParams q;
  flatPreMulFrom(p, scalars, scalarsArePtrs, &q);
  nexrFlatPart* ws = nullptr;
  if (nParts <= kFlatPreMulInlineParts) {
    memcpy(q.parts, parts, (size_t)nParts * sizeof(nexrFlatPart));
  } else {
    res = flatPartsWorkspace(parts, nParts, s, &ws);
    if (res != nexrSuccess) return res;
    q.ext = ws;
  }
  const hipError_t e = launch_flat_premul(dt, q, flatGrid(q.regionBytes, 1), s);
  if (ws) (void)hipFreeAsync(ws, s);
  NEXR_HIP(e);
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrFlatReduceScatterPreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                                  size_t nElts, int datatype, const uint64_t* scalars,
                                                  int scalarsArePtrs, int userFirst, nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  nexrResult_t res = flatReduceScatterCheck(nRanks, inputs, outputs, nElts, datatype, nexrDevPreMulSum, 0, userFirst,
                                            &p, &dt, &op);
  if (res == nexrSuccess) res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (res != nexrSuccess || nElts == 0) return res;
  if (op != nexrDevPreMulSum) {
    NEXR_HIP(launch_flat(dt, op, p, flatGrid(p.regionBytes, nRanks), (hipStream_t)stream));
    return nexrSuccess;
  }
  FlatPreMulParams q;
  flatPreMulFrom(p, scalars, scalarsArePtrs, &q);
  NEXR_HIP(launch_flat_premul(dt, q, flatGrid(q.regionBytes, nRanks), (hipStream_t)stream));
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrFlatReducePreMul(int nRanks, const void* const* inputs, void* output, int root,
                                           size_t nElts, int datatype, const uint64_t* scalars, int scalarsArePtrs,
                                           int userFirst, nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  nexrResult_t res = flatReduceCheck(nRanks, inputs, output, root, nElts, datatype, nexrDevPreMulSum, 0, userFirst, &p,
                                     &dt, &op);
  if (res == nexrSuccess) res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (res != nexrSuccess || nElts == 0) return res;
  if (op != nexrDevPreMulSum) {
    NEXR_HIP(launch_flat(dt, op, p, flatGrid(p.regionBytes, 1), (hipStream_t)stream));
    return nexrSuccess;
  }
  FlatPreMulParams q;
  flatPreMulFrom(p, scalars, scalarsArePtrs, &q);
  NEXR_HIP(launch_flat_premul(dt, q, flatGrid(q.regionBytes, 1), (hipStream_t)stream));
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrFlatTreeAllReducePreMul(int nRanks, const void* const* inputs, void* const* outputs,
                                                  size_t nElts, int datatype, const uint64_t* scalars,
                                                  int scalarsArePtrs, int userFirst,
                                                  const nexrFlatTreeLinks* const* trees, int nTrees,
                                                  const nexrFlatTreePart* parts, int nParts, nexrStream_t stream) {
  FlatTreeParams p;
  int dt, op;
  nexrResult_t res = flatTreeCheck(nRanks, inputs, outputs, nElts, datatype, nexrDevPreMulSum, 0, userFirst, trees,
                                   nTrees, parts, nParts, &p, &dt, &op);
  if (res == nexrSuccess) res = flatScalarsCheck(nRanks, scalars, scalarsArePtrs, datatype);
  if (res != nexrSuccess || nElts == 0) return res;
  hipStream_t s = (hipStream_t)stream;
  if (op != nexrDevPreMulSum) return flatTreeLaunch(p, dt, op, parts, nParts, 0, s);
  FlatTreePreMulParams q;
  memset((void*)&q, 0, sizeof(q));
  memcpy(q.in, p.in, sizeof(q.in));
  memcpy(q.out, p.out, sizeof(q.out));
  memcpy(q.scalars, scalars, (size_t)nRanks * sizeof(uint64_t));
  q.nBytes = p.nBytes;
  q.winBeg = p.winBeg;
  q.winEnd = p.winEnd;
  q.nRanks = p.nRanks;
  q.userFirst = p.userFirst;
  q.preOp = p.preOp;
  q.postOp = p.postOp;
  q.nParts = p.nParts;
  q.nOut = p.nOut;
  q.scalarsArePtrs = scalarsArePtrs ? 1 : 0;
  q.prog[0] = p.prog[0];
  q.prog[1] = p.prog[1];
  nexrFlatTreePart* ws = nullptr;
  if (nParts <= kFlatTreePreMulInlineParts) {
    memcpy(q.parts, parts, (size_t)nParts * sizeof(nexrFlatTreePart));
  } else {
    res = flatTreePartsWorkspace(parts, nParts, s, &ws);
    if (res != nexrSuccess) return res;
    q.ext = ws;
  }
  const hipError_t e = launch_flat_tree_premul(dt, q, flatGrid(q.nBytes, 1), s);
  if (ws) (void)hipFreeAsync(ws, s);
  NEXR_HIP(e);
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrFlatBroadcast(int nRanks, const void* input, void* const* outputs, size_t nBytes,
                                        nexrStream_t stream) {
  if (!input || !outputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  FlatBcastParams p;
  memset((void*)&p, 0, sizeof(p));
  bool any = false;
  for (int r = 0; r < nRanks; r++) {
    if (!outputs[r]) return nexrInvalidArgument;
    if (outputs[r] != input) {
      p.out[r] = (char*)outputs[r];
      any = true;
    }
  }
  if (nBytes == 0 || !any) return nexrSuccess;
  p.in = (const char*)input;
  p.nBytes = p.winEnd = nBytes;
  p.nRanks = nRanks;
  NEXR_HIP(launch_flat_bcast(p, flatGrid(nBytes, 1), (hipStream_t)stream));
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

nexrResult_t groupPlan(int nRanks, const nexrFlatGroupWork* works, int nWorks, int userFirst, int maxWorkgroups,
                       int* launchOf, nexrFlatGroupInfo* info, std::vector<GroupWork>* gwp,
                       std::vector<GroupLaunch>* lp) {
  std::vector<GroupWork>& gw = *gwp;
  std::vector<GroupLaunch>& launches = *lp;
  if (!works || nWorks < 0 || maxWorkgroups < 0) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  std::vector<int> placed((size_t)nWorks, -1);  // work -> its GroupWork
  FlatParams p;
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
    nexrResult_t res = nexrSuccess;
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
      if (w.coll == NEXR_FLAT_GROUP_ALL_REDUCE) {
        res = flatAllReduceCheck(nRanks, w.inputs, w.outputs, w.nElts, w.datatype, w.devRedOp, w.redOpArg, userFirst,
                                 w.parts, w.nParts, &p, &g.dt, &g.op);
      } else if (w.coll == NEXR_FLAT_GROUP_REDUCE_SCATTER) {
        res = flatReduceScatterCheck(nRanks, w.inputs, w.outputs, w.nElts, w.datatype, w.devRedOp, w.redOpArg,
                                     userFirst, &p, &g.dt, &g.op);
      } else if (w.coll == NEXR_FLAT_GROUP_REDUCE) {
        if (!w.outputs || w.root < 0 || w.root >= nRanks) return nexrInvalidArgument;
        res = flatReduceCheck(nRanks, w.inputs, w.outputs[w.root], w.root, w.nElts, w.datatype, w.devRedOp,
                              w.redOpArg, userFirst, &p, &g.dt, &g.op);
      } else {
        return nexrInvalidArgument;
      }
      if (res != nexrSuccess) return res;
      const bool minMax = w.devRedOp == nexrDevMinMax;
      g.isMin = minMax && (w.redOpArg & 1) == 0;
      g.key = w.datatype << 8 | w.devRedOp << 1 | (minMax ? (int)(w.redOpArg & 1) : 0);
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
    uint64_t grid = std::min<uint64_t>((L.items + kBlock / 64 - 1) / (kBlock / 64), gridCap(kBlock));
    if (maxWorkgroups > 0 && grid > (uint64_t)maxWorkgroups) grid = (uint64_t)maxWorkgroups;
    L.grid = (unsigned)grid;
    inf.fillLaunches += L.fills;
    inf.tableBytes += L.tableBytes;
    inf.workgroups += grid;
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
  const nexrResult_t res = groupPlan(nRanks, works, nWorks, userFirst, maxWorkgroups, launchOf, info, &gw, &launches);
  if (res != nexrSuccess) return res;
  hipStream_t s = (hipStream_t)stream;
  std::vector<uint64_t> table;
  for (const GroupLaunch& L : launches) {
    uint32_t poolAt = 0;
    groupTable(L, gw, works, nRanks, &table, &poolAt);
    uint64_t* ws = nullptr;
    if (L.fills) {  // the table by value in short launches ahead of the one: nothing is read after return
      NEXR_HIP(hipMallocAsync((void**)&ws, L.tableBytes, s));
      FlatGroupFill f;
      for (size_t at = 0; at < table.size(); at += kFlatGroupFillWords) {
        f.dst = ws + at;
        f.n = (int)std::min<size_t>(kFlatGroupFillWords, table.size() - at);
        f.pad = 0;
        memcpy(f.words, table.data() + at, (size_t)f.n * 8);
        const hipError_t e = launch_flat_group_fill(f, s);
        if (e != hipSuccess) {
          (void)hipFreeAsync(ws, s);
          return hipFail(e);
        }
      }
    }
    hipError_t e;
    if (L.key == kGroupCopyKey) {
      FlatGroupCopyParams p;
      memset((void*)&p, 0, sizeof(p));
      p.ext = (const char*)ws;
      p.nItems = L.items;
      p.nWorks = (int)L.members.size();
      p.maxOut = L.maxOut;
      if (!ws) memcpy(p.inl, table.data(), L.tableBytes);
      e = launch_flat_group_copy(p, L.grid, s);
    } else {
      const GroupWork& g0 = gw[L.members[0]];
      FlatGroupParams p;
      memset((void*)&p, 0, sizeof(p));
      p.ext = (const char*)ws;
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
      if (!ws) memcpy(p.inl, table.data(), L.tableBytes);
      e = launch_flat_group(g0.dt, g0.op, p, L.grid, s);
    }
    if (ws) (void)hipFreeAsync(ws, s);
    NEXR_HIP(e);
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
  if (nStageIn + nStageOut == 0) {  // zero-copy: the kernel reads and writes the user buffers over the link
    gFhZeroCopy.fetch_add(1, std::memory_order_relaxed);
    gFhWindows.fetch_add(1, std::memory_order_relaxed);
    for (int r = 0; r < io.nIn; r++) devIn[r] = bufs[inIx[r]].dev;
    int m = 0;
    for (int r = 0; r < io.nOut; r++) {
      char* d = outIx[r] < 0 ? nullptr : bufs[outIx[r]].dev;
      if (!io.compact) {
        devOut[m++] = d;
      } else if (d && std::find(devOut, devOut + m, d) == devOut + m) {
        devOut[m++] = d;
      }
    }
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
    // a staged window holds only its own bytes: the kernel addresses `pointer + region offset`
    for (int r = 0; r < io.nIn; r++) {
      const FlatHostBuf& b = bufs[inIx[r]];
      devIn[r] = b.pin ? b.dev : inBase + inStride * (size_t)b.stageIn - wb;
    }
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
  FlatParams p;
  int dt, op;
  const nexrResult_t res = flatAllReduceCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst,
                                              parts, nParts, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  FlatHostIo io;
  io.nIn = io.nOut = nRanks;
  for (int r = 0; r < nRanks; r++) {
    io.in[r] = inputs[r];
    io.out[r] = outputs[r];
  }
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
                       return flatAllReduceLaunch(p, dt, op, parts, nParts, cap, s);
                     });
}

NEXR_API nexrResult_t nexrFlatHostReduceScatter(int nRanks, const void* const* inputs, void* const* outputs,
                                                size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                                int userFirst, nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  const nexrResult_t res =
      flatReduceScatterCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  FlatHostIo io;
  io.nIn = io.nOut = nRanks;
  for (int r = 0; r < nRanks; r++) {
    io.in[r] = inputs[r];
    io.out[r] = outputs[r];
  }
  io.outBytes = (size_t)p.regionBytes;
  io.inBytes = io.outBytes * (size_t)nRanks;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int, uint64_t, uint64_t, uint64_t cap,
                         hipStream_t s) {
                       for (int r = 0; r < nRanks; r++) {
                         p.in[r] = in[r];
                         p.out[r] = out[r];
                       }
                       NEXR_HIP(launch_flat(dt, op, p, flatGrid(p.regionBytes, nRanks, cap), s));
                       return nexrSuccess;
                     });
}

NEXR_API nexrResult_t nexrFlatHostReduce(int nRanks, const void* const* inputs, void* output, int root, size_t nElts,
                                         int datatype, int devRedOp, uint64_t redOpArg, int userFirst,
                                         nexrStream_t stream) {
  FlatParams p;
  int dt, op;
  const nexrResult_t res =
      flatReduceCheck(nRanks, inputs, output, root, nElts, datatype, devRedOp, redOpArg, userFirst, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  FlatHostIo io;
  io.nIn = nRanks;
  io.nOut = 1;
  for (int r = 0; r < nRanks; r++) io.in[r] = inputs[r];
  io.out[0] = output;
  io.inBytes = io.outBytes = (size_t)p.regionBytes;
  io.windowed = true;
  return flatHostRun(io, (hipStream_t)stream,
                     [&](const char* const* in, char* const* out, int, uint64_t wb, uint64_t we, uint64_t cap,
                         hipStream_t s) {
                       for (int r = 0; r < nRanks; r++) p.in[r] = in[r];
                       p.out[root] = out[0];
                       p.winBeg = wb;
                       p.winEnd = we;
                       NEXR_HIP(launch_flat(dt, op, p, flatGrid(we - wb, 1, cap), s));
                       return nexrSuccess;
                     });
}

NEXR_API nexrResult_t nexrFlatHostTreeAllReduce(int nRanks, const void* const* inputs, void* const* outputs,
                                                size_t nElts, int datatype, int devRedOp, uint64_t redOpArg,
                                                int userFirst, const nexrFlatTreeLinks* const* trees, int nTrees,
                                                const nexrFlatTreePart* parts, int nParts, nexrStream_t stream) {
  FlatTreeParams p;
  int dt, op;
  const nexrResult_t res = flatTreeCheck(nRanks, inputs, outputs, nElts, datatype, devRedOp, redOpArg, userFirst,
                                         trees, nTrees, parts, nParts, &p, &dt, &op);
  if (res != nexrSuccess || nElts == 0) return res;
  FlatHostIo io;
  io.nIn = io.nOut = nRanks;
  for (int r = 0; r < nRanks; r++) {
    io.in[r] = inputs[r];
    io.out[r] = outputs[r];
  }
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
                       return flatTreeLaunch(p, dt, op, parts, nParts, cap, s);
                     });
}

NEXR_API nexrResult_t nexrFlatHostBroadcast(int nRanks, const void* input, void* const* outputs, size_t nBytes,
                                            nexrStream_t stream) {
  if (!input || !outputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  FlatHostIo io;
  bool any = false;
  for (int r = 0; r < nRanks; r++) {
    if (!outputs[r]) return nexrInvalidArgument;
    io.out[r] = outputs[r] != input ? outputs[r] : nullptr;
    any = any || io.out[r];
  }
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
  if (!inputs || !outputs) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS) return nexrInvalidArgument;
  if (nBytes > (size_t)-1 / (size_t)nRanks) return nexrInvalidArgument;  // an output's nRanks * nBytes bytes
  FlatHostIo io;
  for (int r = 0; r < nRanks; r++) {
    if (!inputs[r] || !outputs[r]) return nexrInvalidArgument;
    io.in[r] = inputs[r];
    io.out[r] = outputs[r];
  }
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
                       for (int r = 0; r < nRanks; r++) {
                         p.in[r] = in[r];
                         p.out[r] = out[r];
                         // Pageable outputs all name the one staged output, which the kernel therefore
                         // stores once per pageable rank (the same bytes, in device memory: up to n times
                         // the device writes, none over the link). The reference's inPlace, per rank: a
                         // staged buffer never lies inside another
                         if ((uintptr_t)in[r] == (uintptr_t)out[r] + (uintptr_t)r * nBytes) p.inPlace |= 1ull << r;
                       }
                       p.nBytes = nBytes;
                       p.nRanks = nRanks;
                       unsigned grid = symChunkGrid(nBytes, 1, nRanks);
                       if (cap > 0 && grid > cap) grid = (unsigned)cap;
                       NEXR_HIP(launch_sym_all_gather(p, grid, s));
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
  if (!bytes || nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS || maxBlocks < 1 || maxBlocks > NEXR_SYM_LL_MAX_BLOCKS)
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
  if (const char* e = getenv("NEXR_TEST_SYM_LL_RESIDENT"))
    if (*e) {
      *resident = strtoll(e, nullptr, 10);
      return nexrSuccess;
    }
  constexpr int kDevs = 16;
  static std::atomic<int64_t> cache[3][kDevs][nexrNumTypes];
  int dev = 0;
  NEXR_HIP(hipGetDevice(&dev));
  const bool cached = dev >= 0 && dev < kDevs;
  if (cached) {
    const int64_t v = cache[coll][dev][dt].load(std::memory_order_relaxed);
    if (v > 0) {
      *resident = v;
      return nexrSuccess;
    }
  }
  int cus = 0, blocks = 0;
  NEXR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  NEXR_HIP(sym_ll_blocks_per_cu(coll, dt, &blocks));
  if (blocks > 4) blocks = 4;
  if (blocks > 1) blocks--;
  *resident = (int64_t)blocks * cus;
  if (cached && *resident > 0) cache[coll][dev][dt].store(*resident, std::memory_order_relaxed);
  return nexrSuccess;
}

// The host side of the three calls. coll: 0 all-reduce (count elements per buffer), 1 reduce-scatter (count
// elements per chunk), 2 all-gather (count bytes, esz 1).
nexrResult_t symLL(int coll, int nRanks, const void* const* inputs, void* const* outputs, size_t count, int datatype,
                   void* const* windows, size_t windowBytes, int nBlocks, uint32_t* status, uint32_t timeoutUs,
                   nexrStream_t stream) {
  if (!inputs || !outputs || !windows) return nexrInvalidArgument;
  if (nRanks < 2 || nRanks > NEXR_SYM_MAX_RANKS || nBlocks < 0 || nBlocks > NEXR_SYM_LL_MAX_BLOCKS)
    return nexrInvalidArgument;
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
  p.timeoutTicks = (uint64_t)(timeoutUs ? timeoutUs : 1000000u) * 100u;  // s_memrealtime: 100 MHz
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

NEXR_API nexrResult_t nexrReduceCopyLL128(const void* src, int srcIsInput, int nRecv, const void* const* recvWire,
                                          const uint64_t* recvFlags, void* dst, int nSend, void* const* sendWire,
                                          const uint64_t* sendFlags, size_t nElts, int datatype, int devRedOp,
                                          uint64_t redOpArg, int postOp, uint32_t* status, uint32_t timeoutUs,
                                          nexrStream_t stream) {
  if (nRecv < 0 || nRecv > NEXR_MAX_SRCS || nSend < 0 || nSend > NEXR_MAX_DSTS) return nexrInvalidArgument;
  if ((!src && nRecv == 0) || (!dst && nSend == 0)) return nexrInvalidArgument;
  if (datatype < 0 || datatype >= nexrNumTypes || datatype == nexrFloat8e4m3 || datatype == nexrFloat8e5m2)
    return nexrInvalidArgument;
  if (devRedOp < 0 || devRedOp >= nexrNumDevRedOps) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && !isInteger(datatype)) return nexrInvalidArgument;
  if (devRedOp == nexrDevSumPostDiv && (redOpArg & 1) != 0 && typeSize(datatype) == 1) {  // as validate()
    uint32_t divisor = (uint32_t)(redOpArg >> 1);
    if (divisor == 0) divisor = 1;
    if ((int8_t)divisor == 0) return nexrInvalidArgument;
  }
  if ((nRecv && (!recvWire || !recvFlags)) || (nSend && (!sendWire || !sendFlags))) return nexrInvalidArgument;
  if (nElts == 0) return nexrSuccess;
  LL128Params a;
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
  a.timeoutTicks = (uint64_t)(timeoutUs ? timeoutUs : 1000000u) * 100u;
  a.nRecv = nRecv;
  a.nSend = nSend;
  a.srcIsInput = srcIsInput ? 1 : 0;
  a.postOp = postOp ? 1 : 0;
  llSemantics(&datatype, &devRedOp, &a.srcIsInput, &a.postOp, &a.firstWins);
  const uint64_t nUnits = (nElts * typeSize(datatype) + kLL128SliceData - 1) / kLL128SliceData * 128;
  uint64_t grid = (nUnits + kLL128TileUnits - 1) / kLL128TileUnits;
  if (grid > (1u << 20)) grid = 1u << 20;
  NEXR_HIP(launch_ll128(datatype, a, devRedOp, (int)grid, (hipStream_t)stream));
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrSetSemantics(int mode) {
  if (mode < 0 || mode >= nexrNumSemantics) return nexrInvalidArgument;
  gSemantics.store(mode, std::memory_order_relaxed);
  return nexrSuccess;
}

NEXR_API nexrResult_t nexrGetSemantics(int* mode) {
  if (mode == nullptr) return nexrInvalidArgument;
  *mode = semantics();
  return nexrSuccess;
}

NEXR_API size_t nexrTypeSize(int datatype) { return typeSize(datatype); }

NEXR_API const char* nexrGetErrorString(nexrResult_t result) {
  switch (result) {
    case nexrSuccess: return "no error";
    case nexrUnhandledCudaError: return "unhandled HIP error (run with nexrGetLastHipError for details)";
    case nexrSystemError: return "unhandled system error";
    case nexrInternalError: return "internal error";
    case nexrInvalidArgument: return "invalid argument";
    case nexrInvalidUsage: return "invalid usage";
    case nexrRemoteError: return "remote process exited or there was a network error";
    case nexrInProgress: return "operation in progress";
    default: return "unknown result code";
  }
}

NEXR_API int nexrGetVersion(void) {
  return NEXR_VERSION_MAJOR * 10000 + NEXR_VERSION_MINOR * 100 + NEXR_VERSION_PATCH;
}

NEXR_API int nexrGetLastHipError(void) { return tLastHipError; }

}  // extern "C"
