// nexr_exchange_v_checks.h — the checks of the all-to-all with a count per pair that need no device, shared by
// nexrFlatAllToAllv (nexr_flat_api.cpp) and nexrRingAllToAllv (nexr_ring.cpp, at any rank count): the half-open range
// rule and the bound on a capacity stand here and nowhere else. The reduce-scatter and the all-gather with a count
// per rank (nexrFlatReduceScatterv, nexrFlatAllGatherv and their ring entries) share them, with n counts. The
// exchanges of a fixed size (nexrFlatAllToAll, nexrFlatAllToAll2D, nexrFlatAllGather2D and their ring entries) take
// the range rule from fixedRangesOk.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace nexr_exchange_v {

// A capacity is at most this many bytes, so that 64 admitted counts cannot wrap a 64-bit sum.
constexpr uint64_t kMaxBytes = (uint64_t)1 << 56;

struct Range {  // half-open; an empty range meets nothing, one that ends where the other begins does not meet it
  uintptr_t beg, end;
  bool meets(const Range& o) const { return beg < end && o.beg < o.end && beg < o.end && o.beg < end; }
};

// The checks that read no count: every capacity within kMaxBytes and inside the address space, a buffer wherever a
// capacity is not 0, no output range meeting an input range or another output range (in place is not offered; inputs
// may alias each other) and, with device counts, none meeting the counts (n * n of them, or countWords) or the
// status word.
inline bool buffersOk(int n, const void* const* in, void* const* out, const size_t* inElts, const size_t* outElts,
                      size_t esz, const uint64_t* counts, const uint32_t* status, bool deviceCounts,
                      size_t countWords = 0) {
  auto range = [esz](const void* p, size_t elts) { return Range{(uintptr_t)p, (uintptr_t)p + elts * esz}; };
  for (int r = 0; r < n; r++) {
    if (inElts[r] > kMaxBytes / esz || outElts[r] > kMaxBytes / esz) return false;
    if ((inElts[r] && !in[r]) || (outElts[r] && !out[r])) return false;
    if (range(in[r], inElts[r]).end < (uintptr_t)in[r] || range(out[r], outElts[r]).end < (uintptr_t)out[r]) return false;
  }
  const Range cnt = {(uintptr_t)counts, (uintptr_t)counts + (countWords ? countWords : (uintptr_t)n * n) * 8u};
  const Range word = {(uintptr_t)status, (uintptr_t)status + 4u};
  for (int d = 0; d < n; d++) {
    const Range o = range(out[d], outElts[d]);
    for (int s = 0; s < n; s++)
      if (o.meets(range(in[s], inElts[s]))) return false;
    for (int e = 0; e < d; e++)
      if (o.meets(range(out[e], outElts[e]))) return false;
    if (deviceCounts && (o.meets(cnt) || o.meets(word))) return false;
  }
  return true;
}

// The range rule for a fixed length per side: every in[s] is inLen bytes and every out[d] outLen bytes. No output
// range may meet an input range (in place is not offered) nor, with amongOutputs, another output range. A length of
// 0 meets nothing. These callers put no bound on a length, so an end is compared as the address arithmetic gives
// it, without Range's order of beg and end.
inline bool fixedRangesOk(int n, const void* const* in, void* const* out, uintptr_t inLen, uintptr_t outLen,
                          bool amongOutputs) {
  auto meets = [](const void* a, uintptr_t aLen, const void* b, uintptr_t bLen) {
    return (uintptr_t)a < (uintptr_t)b + bLen && (uintptr_t)b < (uintptr_t)a + aLen;
  };
  for (int d = 0; d < n; d++) {
    for (int s = 0; s < n; s++)
      if (meets(out[d], outLen, in[s], inLen)) return false;
    for (int e = 0; e < d && amongOutputs; e++)
      if (meets(out[d], outLen, out[e], outLen)) return false;
  }
  return true;
}

// Whether host counts keep inside the capacities: every count, every row sum, every column sum. A sum is compared
// as it grows, so none wraps at any rank count. colSum[d] (n words of the caller's) ends as column d's sum.
inline bool countsFit(int n, const uint64_t* counts, const size_t* inElts, const size_t* outElts, uint64_t* colSum) {
  for (int d = 0; d < n; d++) colSum[d] = 0;
  for (int s = 0; s < n; s++) {
    uint64_t row = 0;
    for (int d = 0; d < n; d++) {
      const uint64_t c = counts[(size_t)s * n + d];
      if (c > inElts[s] || c > outElts[d]) return false;
      row += c;
      colSum[d] += c;
      if (row > inElts[s] || colSum[d] > outElts[d]) return false;
    }
  }
  return true;
}

// The same for a count per rank (host counts). scatter: piece d goes to out[d] alone and every in[r] holds all of
// them (the reduce-scatter); else piece r comes from in[r] alone and every out[t] holds all of them (the all-gather).
inline bool piecesFit(int n, const uint64_t* counts, const size_t* inElts, const size_t* outElts, bool scatter,
                      uint64_t* total) {
  const size_t* own = scatter ? outElts : inElts;
  const size_t* all = scatter ? inElts : outElts;
  uint64_t least = ~(uint64_t)0;
  for (int r = 0; r < n; r++) least = all[r] < least ? all[r] : least;
  *total = 0;
  for (int d = 0; d < n; d++) {
    if (counts[d] > own[d]) return false;
    *total += counts[d];
    if (*total > least) return false;
  }
  return true;
}

}  // namespace nexr_exchange_v
