// nexr_flat_exchange_v.hip — the personalised exchange with a count per pair in ONE launch (nexrFlatAllToAllv), for
// gfx950. Included at the end of nexr_ll.hip behind nexr_flat_alltoall.hip: the LL / LL128 object stays the one code
// object beside the per-datatype ones, and the helpers of the flat files before it (kFlatPiece, c_tbl / tbl_ld,
// flat_alltoall_arg, the unaligned pack types) are shared by inclusion order only.
//
// What it computes. counts[s * n + d] elements of 1 << shift bytes go from rank s to rank d, packed on both sides:
//   sendOff(s, d) = sum of counts[s * n + d'] over d' < d,   recvOff(d, s) = sum of counts[s' * n + d] over s' < s,
//   out[d][recvOff(d, s) + i] = in[s][sendOff(s, d) + i]     (offsets in bytes here).
// The matrix is read by the kernel alone: from the kernel arguments (host counts of up to kFlatExchangeVInlineRanks
// ranks), from the call's stream-ordered workspace (host counts beyond that), or from the caller's device memory
// (device counts, whatever the stream wrote last). The host never needs the values to plan the launch.
//
// Two phases in one launch.
//   Prologue, once per workgroup, 16 * n * n bytes of dynamic LDS (two n x n tables of 64-bit words: 64 KiB at 64
//     ranks, 1 KiB at 8, so a small communicator keeps its occupancy). Wave w owns rows w, w + 4, ...: lane d holds
//     counts[s * n + d], an inclusive scan over the wave (six ds_bpermute steps per half, no LDS allocated for it)
//     gives sendOff(s, .) and the row's total. A barrier, then the same wave owns columns w, w + 4, ...: lane s holds
//     counts[s * n + d], the scan gives recvOff(d, .) and the output row's total, and the lane writes
//       R[d][s] = recvOff(d, s)  (s >= 1; R[d][0], always zero, holds the row's total instead), and
//       S[d][s] = in[s] + sendOff(s, d) - recvOff(d, s): the address that, plus an offset in out[d], is its source.
//     The verdict: a count above either of its two capacities is a violation by itself (the host keeps every
//     capacity at or below 2^56 bytes, so no sum of 64 admitted counts wraps); so is a row total above in's capacity
//     or a column total above out's. A wave that saw one writes ~0 as the total of every row it owns. A second
//     barrier ends the prologue, and every wave reads the n totals (lane d: row d): any ~0 and the whole launch
//     writes nothing but *status = 1. The verdict is a pure function of the matrix: every workgroup reaches the
//     same one, with no atomics, no polls and no cross-workgroup traffic. (Two barriers, not one: S[d][s] needs the
//     row scan of another wave.)
//   Copy, persistent. The items are the kFlatPiece pieces of every packed output row, row after row: lane d's
//     inclusive scan of the rows' piece counts stays in registers, so an item's row is a ballot and a popcount, and
//     the item count is exact whatever the grid was sized from (capacities, with device counts): a wave whose item
//     number is at or above it leaves. A wave takes one piece, so consecutive waves write consecutive addresses
//     whatever the block sizes are. Each lane holds two 16-byte packs 1024 bytes apart. It finds the block of a pack
//     by a branch-free upper-bound search over R[d][.] (log2 n steps, six at the most), forms S[d][s] + o, and
//       a pack wholly inside one block is one unaligned 16-byte load and store;
//       a pack that meets a block boundary (n - 1 per row at the most, blocks under 16 bytes included) or the row's
//       end is copied byte by byte by its own lane, stepping over empty blocks.
// User pointers have no alignment; offsets are 64-bit; the cache policy is plain; no scratch.

namespace nexr {

__device__ __forceinline__ uint64_t xv_from_lane(uint32_t from, uint64_t v) {  // every lane active
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(from << 2), (int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(from << 2), (int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

// The inclusive prefix sum over the 64 lanes.
__device__ __forceinline__ uint64_t xv_scan(uint32_t lane, uint64_t v) {
#pragma unroll
  for (uint32_t k = 1; k < 64; k <<= 1) {
    const uint64_t below = xv_from_lane((lane - k) & 63u, v);
    if (lane >= k) v += below;
  }
  return v;
}

__device__ __forceinline__ uint64_t xv_lane(uint64_t v, uint32_t l) {  // l wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(kBlock) void flat_exchange_v_kernel(FlatExchangeVParams P) {
  extern __shared__ uint64_t xv_lds[];
  constexpr uint32_t kWaves = kBlock / 64;
  constexpr uint32_t kIn = offsetof(FlatExchangeVParams, in), kOut = offsetof(FlatExchangeVParams, out);
  constexpr uint32_t kInElts = offsetof(FlatExchangeVParams, inElts), kOutElts = offsetof(FlatExchangeVParams, outElts);
  constexpr uint64_t kBad = ~(uint64_t)0;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks, shift = (uint32_t)P.shift;
  uint64_t* R = xv_lds;          // [d][s]: recvOff(d, s) in bytes; [d][0]: the row's total
  uint64_t* S = xv_lds + n * n;  // [d][s]: sendOff(s, d), then the source address less the output offset
  c_tbl* cnt = P.ext ? (c_tbl*)(uintptr_t)P.ext
                     : (c_tbl*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FlatExchangeVParams, inl);
  const bool has = lane < n;
  const uint32_t mine = has ? lane : 0u;
  // lane r keeps rank r's capacities (elements) and input pointer
  const uint64_t inCap = flat_alltoall_arg(kInElts + 8u * mine), outCap = flat_alltoall_arg(kOutElts + 8u * mine);
  const uint64_t inPtr = flat_alltoall_arg(kIn + 8u * mine);

  bool bad = false;
  for (uint32_t s = wave; s < n; s += kWaves) {  // rows: lane d
    const uint64_t c = has ? tbl_ld<uint64_t>(cnt + 8ull * (s * n + lane)) : 0;
    const uint64_t cap = xv_lane(inCap, s);
    bad |= c > cap || c > outCap;
    const uint64_t bytes = c << shift;
    const uint64_t incl = xv_scan(lane, bytes);
    bad |= xv_lane(incl, 63) > cap << shift;
    if (has) S[lane * n + s] = incl - bytes;
  }
  __syncthreads();
  for (uint32_t d = wave; d < n; d += kWaves) {  // columns: lane s
    const uint64_t c = has ? tbl_ld<uint64_t>(cnt + 8ull * (lane * n + d)) : 0;
    const uint64_t cap = xv_lane(outCap, d);
    bad |= c > cap || c > inCap;
    const uint64_t bytes = c << shift;
    const uint64_t incl = xv_scan(lane, bytes);
    const uint64_t total = xv_lane(incl, 63);
    bad |= total > cap << shift;
    const uint64_t recvOff = incl - bytes;
    if (has) {
      S[d * n + lane] = inPtr + S[d * n + lane] - recvOff;
      R[d * n + lane] = lane ? recvOff : total;
    }
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0)
    for (uint32_t d = wave; d < n; d += kWaves) R[d * n] = kBad;
  __syncthreads();

  const uint64_t total = has ? R[lane * n] : 0;  // lane d: row d
  const bool violated = __builtin_amdgcn_ballot_w64(has && total == kBad) != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && P.status) *P.status = violated ? 1u : 0u;
  if (violated) return;
  const uint64_t pieceEnd = xv_scan(lane, (total + (kFlatPiece - 1)) / kFlatPiece);  // lanes beyond n: the item count
  const uint64_t nItems = xv_lane(pieceEnd, 63);
  const uint64_t nWaves = (uint64_t)gridDim.x * kWaves;
  uint32_t top = 1;  // the first step of the search: the largest power of two below n
  while (top * 2u < n) top *= 2u;

  for (uint64_t it = (uint64_t)blockIdx.x * kWaves + wave; it < nItems; it += nWaves) {
    const uint32_t d = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pieceEnd <= it));  // below n
    const uint64_t rowBytes = xv_lane(total, d);
    const uint64_t first = xv_lane(pieceEnd, d) - (rowBytes + (kFlatPiece - 1)) / kFlatPiece;
    const uint64_t pBeg = (it - first) * kFlatPiece;
    char* dst = (char*)(uintptr_t)flat_alltoall_arg(kOut + 8u * d);
    const uint64_t* Rd = R + d * n;
    const uint64_t* Sd = S + d * n;
    uint32_t blk[2];
    uint64_t end[2];
    bool whole[2], bytes[2];
    u32x4 v[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint64_t o = pBeg + lane * 16u + (uint32_t)u * (kFlatPiece / 2);
      const bool in = o < rowBytes;
      uint32_t s = 0;  // the last block that begins at or before o: it holds o, the empty ones before it do not
      for (uint32_t step = top; step; step >>= 1) {
        const uint32_t t = s + step;
        if (in && t < n && Rd[t] <= o) s = t;
      }
      blk[u] = s;
      end[u] = in && s + 1u < n ? Rd[s + 1u] : rowBytes;
      whole[u] = in && o + 16u <= end[u];
      bytes[u] = in && !whole[u];
      v[u] = (u32x4)0u;
      if (whole[u]) v[u] = *(g_cu32x4_a1*)(uintptr_t)(Sd[s] + o);
    }
#pragma unroll
    for (int u = 0; u < 2; u++)
      if (whole[u]) *(g_u32x4_a1*)(dst + pBeg + lane * 16u + u * (kFlatPiece / 2)) = v[u];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (!bytes[u]) continue;
      const uint64_t o = pBeg + lane * 16u + (uint32_t)u * (kFlatPiece / 2);
      const uint64_t stop = o + 16u < rowBytes ? o + 16u : rowBytes;
      uint32_t s = blk[u];
      uint64_t e = end[u];
      for (uint64_t ob = o; ob < stop; ob++) {
        while (ob >= e) {  // the next block that holds a byte; the last one ends at rowBytes, above ob
          s++;
          e = s + 1u < n ? Rd[s + 1u] : rowBytes;
        }
        *(g_u8*)(dst + ob) = *(g_cu8*)(uintptr_t)(Sd[s] + ob);
      }
    }
  }
}

hipError_t launch_flat_exchange_v(const FlatExchangeVParams& p, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<FlatExchangeVParams*>(&p)};
  const size_t lds = (size_t)16 * (size_t)p.nRanks * (size_t)p.nRanks;
  return hipLaunchKernel((const void*)&flat_exchange_v_kernel, dim3(grid), dim3(kBlock), args, lds, s);
}

}  // namespace nexr
