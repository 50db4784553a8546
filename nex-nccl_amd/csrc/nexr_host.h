// nexr_host.h — what the host translation units of libnexr.so share (nexr_api.cpp defines it all, nexr_flat_api.cpp
// and nexr_steps_api.cpp use it). Declarations only: everything with state (the registration cache, the staging
// pool, the counters, the last HIP error) keeps its one definition in nexr_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "nexr_internal.h"

namespace nexr {

// Records e as the thread's last HIP error (nexrGetLastHipError) and returns nexrUnhandledCudaError.
nexrResult_t hipFail(hipError_t e);
#define NEXR_HIP(call)                          \
  do {                                          \
    hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hipFail(e_);   \
  } while (0)

size_t typeSize(int dt);  // 0: not a datatype
bool isInteger(int dt);
long envLong(const char* name, long dflt);

// The datatype, device op and SumPostDiv divisor that every reduce-copy entry takes.
bool typeOpOk(int datatype, int devRedOp, uint64_t redOpArg);
// The ticks a kernel polls before it gives up: timeoutUs, or one second for 0.
uint64_t pollTicks(uint32_t timeoutUs);

// Workgroups of one kernel the current device keeps resident (blocks per CU x CUs). The caller names the kernel
// and holds what is known about it: the cache slot of that kernel (a function-local static of the caller), the
// occupancy query with its two arguments, the cap on the query's answer per CU (0: none) and whether one is
// taken off it. hook: an environment variable that, when set, is taken as the answer; read per call (tests set
// it between calls), before any HIP call.
constexpr int kResidentDevs = 16;
using ResidentSlot = std::atomic<int64_t>[kResidentDevs];
struct ResidentLookup {
  const char* hook;
  ResidentSlot* slot;
  hipError_t (*blocksPerCu)(int a, int b, int* blocks);
  int a, b;
  int capPerCu;
  bool lessOne;
};
nexrResult_t residentWorkgroups(const ResidentLookup& k, int64_t* resident);

int semantics();  // nexrSetSemantics / NEXR_SEMANTICS
void llSemantics(int* dt, int* op, int* srcIsInput, int* postOp, int* firstWins);

uint64_t gridCap(int block);  // the workgroups of `block` lanes that HIP's work-item limit admits
uint64_t hostGrid();          // the grid's cap where a kernel reads or writes host memory; 0: none

// The registration cache (nexrHostRegister): true and *dev where [p, p + bytes) lies inside one registration.
bool regLookup(const void* p, size_t bytes, void** dev);

// A staging ring of the process-wide pool: two device slots, a stream for the copies out and an event pair per slot.
struct HostStage {
  int device = -1;
  char* buf = nullptr;
  size_t slotBytes = 0;  // bytes per slot
  hipStream_t out = nullptr;
  hipEvent_t kernelDone[2] = {nullptr, nullptr};
  hipEvent_t outDone[2] = {nullptr, nullptr};
};
// A ring checked out by stageFor; handed back, drained, when the lease ends.
struct StageLease {
  HostStage* st = nullptr;
  hipStream_t caller = nullptr;
  ~StageLease();
};
nexrResult_t stageFor(size_t slotBytes, hipStream_t caller, StageLease* lease);

// hipMemcpyAsync to or from a host buffer that may run past the end of the pinned range it begins in, in pieces.
hipError_t hostCopyPieces(char* dev, char* host, size_t bytes, bool toDevice, hipStream_t s);

}  // namespace nexr
