// nexr_flat_scatter_v.hip — the reduce-scatter and the all-gather with a count per rank in ONE launch
// (nexrFlatReduceScatterv, nexrFlatAllGatherv), for gfx950. Included at the end of nexr_ll.hip behind
// nexr_flat_exchange_v.hip: the LL / LL128 object stays the one code object beside the per-datatype ones, and the
// helpers of the flat files before it (flat_fold and the element accesses of nexr_flat.hip, flat_alltoall_arg, the
// wave scan xv_scan / xv_lane, the unaligned pack types) are shared by inclusion order only.
//
// What they compute. counts[d] elements make piece d, off(d) = sum of counts[d'] over d' < d, both sides packed in
// rank order:
//   reduce-scatter-v: out[d][e], e < counts[d], is the ring reduce with root d over in[r] + off(d): flat_fold's
//     chain started at rank d + 1, the bytes of nexrFlatReduce on that piece;
//   all-gather-v:     out[t][off(r) + i] = in[r][i], i < counts[r], for every t (a bit copy at any alignment).
// The n <= 64 counts are read by the kernel alone: from the kernel arguments (host counts; 64 words fit at any
// rank count, so there is no workspace and no fill launch) or from the caller's device memory (device counts,
// whatever the stream wrote last).
//
// Prologue, per wave, in registers: lane d holds counts[d] and rank d's two capacities; one inclusive scan over
// the wave (xv_scan: six ds_bpermute steps per half, no LDS allocated, no barrier) gives off(d) and the total.
// A lane's own count above the capacity of its piece, or the total above the capacity of the lane's other buffer,
// is a violation; a ballot makes it the wave's verdict. The host keeps every capacity at or below 2^56 bytes, so
// no sum of 64 admitted counts wraps, and a count that is not admitted is a violation by itself. The verdict is a
// pure function of the counts and capacities: every wave of every workgroup reaches the same one, with no
// atomics and no cross-workgroup traffic. Workgroup 0 writes *status; on a violation nothing else is written.
//
// Items. A second scan, over the rows' piece counts ceil(counts[d] * esz / 2048), stays in registers: an item's
// row is a ballot and a popcount, and the item count is exact whatever the grid was sized from (capacities, with
// device counts): a wave whose item number is at or above it leaves. Row after row, so consecutive waves write
// consecutive addresses. Each lane holds two 16-byte packs 1024 bytes apart.
//   reduce-scatter-v: the input offset is off(d) * esz + position, the output offset is position: a piece's phase
//     in the inputs is arbitrary and differs from the output's, so every pack access is the unaligned-capable
//     form; the row's last bytes below a pack go one element per lane. The start rank is wave-uniform.
//   all-gather-v: a pack is loaded once and stored to all n outputs, whose pointers are scalar loads from the
//     kernel arguments; the block's end below a pack goes one byte per lane, in the wave of the block's last piece.
// Offsets are 64-bit; the cache policy is plain; no LDS, no scratch.

namespace nexr {

// Lane d: off(d) and counts[d] in bytes. False: a violation (the launch writes nothing but the status).
template <bool kGather>
__device__ __forceinline__ bool sv_plan(const FlatScatterVParams& P, uint32_t lane, uint64_t* offBytes,
                                        uint64_t* bytes) {
  constexpr uint32_t kCounts = offsetof(FlatScatterVParams, counts);
  constexpr uint32_t kInElts = offsetof(FlatScatterVParams, inElts), kOutElts = offsetof(FlatScatterVParams, outElts);
  constexpr uint32_t kOwn = kGather ? kInElts : kOutElts;    // the buffer that holds the lane's piece alone
  constexpr uint32_t kAll = kGather ? kOutElts : kInElts;    // the lane's buffer that holds every piece
  const uint32_t n = (uint32_t)P.nRanks, sh = (uint32_t)P.eszShift;
  const bool has = lane < n;
  const uint32_t mine = has ? lane : 0u;
  uint64_t c = 0;
  if (has) c = P.ext ? *(g_cu64*)(uintptr_t)(P.ext + lane) : flat_alltoall_arg(kCounts + 8u * lane);
  const uint64_t own = flat_alltoall_arg(kOwn + 8u * mine), all = flat_alltoall_arg(kAll + 8u * mine);
  const uint64_t incl = xv_scan(lane, c);
  const uint64_t total = xv_lane(incl, 63);
  const bool violated = __builtin_amdgcn_ballot_w64(has && (c > own || total > all)) != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && P.status) *P.status = violated ? 1u : 0u;
  *offBytes = (incl - c) << sh;
  *bytes = c << sh;
  return !violated;
}

// The rows' pieces as items: row `d` and the piece's first byte in it, for the wave-uniform item number `it`.
struct SvItems {
  uint64_t pieceEnd;  // lane d: the items up to and including row d; lanes beyond n: the item count
  uint64_t nItems;
  __device__ __forceinline__ void init(uint32_t lane, uint64_t bytes) {
    pieceEnd = xv_scan(lane, (bytes + (kFlatPiece - 1)) / kFlatPiece);
    nItems = xv_lane(pieceEnd, 63);
  }
  __device__ __forceinline__ uint32_t row(uint64_t it, uint64_t bytes, uint64_t* rowBytes, uint64_t* pBeg) const {
    const uint32_t d = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pieceEnd <= it));  // below n
    *rowBytes = xv_lane(bytes, d);
    const uint64_t first = xv_lane(pieceEnd, d) - (*rowBytes + (kFlatPiece - 1)) / kFlatPiece;
    *pBeg = (it - first) * kFlatPiece;
    return d;
  }
};

template <int D, int OP, bool IsMin>
__device__ __forceinline__ void scatter_v_run(const FlatScatterVParams& P) {
  constexpr uint32_t esz = 16 / Ty<D>::EPP;
  constexpr uint32_t kOut = offsetof(FlatScatterVParams, out);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks, shift = (uint32_t)P.shift;
  uint64_t offBytes, bytes;
  if (!sv_plan<false>(P, lane, &offBytes, &bytes)) return;
  SvItems items;
  items.init(lane, bytes);
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < items.nItems; it += nWaves) {
    uint64_t rowBytes, pBeg;
    const uint32_t d = items.row(it, bytes, &rowBytes, &pBeg);
    const uint64_t inBase = xv_lane(offBytes, d);  // piece d of every input
    char* dst = (char*)(uintptr_t)flat_alltoall_arg(kOut + 8u * d);
    uint32_t first = d + 1u + shift;  // the chain starts at d + 1 (the rank after it under shipped semantics)
    first = first >= n ? first - n : first;  // d + 1 <= n and shift < n: below 2n
    const uint64_t mine = pBeg + lane * 16u;
    {
      bool valid[2];
      u32x4 out[2];
#pragma unroll
      for (int u = 0; u < 2; u++) valid[u] = mine + (uint64_t)u * (kFlatPiece / 2) + 16u <= rowBytes;
      flat_fold<FlatScatterVParams, D, OP, IsMin, 2, kFlatPiece / 2, false>(P, first, inBase + mine, valid, out);
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (valid[u]) *(g_u32x4_a1*)(dst + mine + u * (kFlatPiece / 2)) = out[u];
    }
    const uint32_t tail = (uint32_t)(rowBytes & 15u) / esz;
    if (pBeg + kFlatPiece >= rowBytes && tail != 0) {  // the row's last bytes below a pack: one element per lane
      const uint64_t o = (rowBytes & ~(uint64_t)15) + lane * esz;
      bool valid[1] = {lane < tail};
      u32x4 out[1];
      flat_fold<FlatScatterVParams, D, OP, IsMin, 1, 0, true>(P, first, inBase + o, valid, out);
      if (valid[0]) flat_st_elem<esz>(dst + o, out[0]);
    }
  }
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void flat_scatter_v_kernel(FlatScatterVParams P) {
  if constexpr (OP == nexrDevMinMax) {
    if ((P.redArg & 1) == 0) scatter_v_run<D, OP, true>(P);
    else scatter_v_run<D, OP, false>(P);
  } else {
    scatter_v_run<D, OP, false>(P);
  }
}

__global__ __launch_bounds__(kBlock) void flat_gather_v_kernel(FlatScatterVParams P) {
  constexpr uint32_t kIn = offsetof(FlatScatterVParams, in), kOut = offsetof(FlatScatterVParams, out);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks;
  uint64_t offBytes, bytes;
  if (!sv_plan<true>(P, lane, &offBytes, &bytes)) return;
  SvItems items;
  items.init(lane, bytes);
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < items.nItems; it += nWaves) {
    uint64_t rowBytes, pBeg;
    const uint32_t r = items.row(it, bytes, &rowBytes, &pBeg);
    const char* src = (const char*)(uintptr_t)flat_alltoall_arg(kIn + 8u * r);
    const uint64_t outBase = xv_lane(offBytes, r);  // block r of every output
    const uint64_t mine = pBeg + lane * 16u;
    // the block's end below a pack, in the wave that holds the block's last piece: one byte per lane, loaded with
    // the packs (a single lane walking its up to 15 bytes waits for one load after the other: DESIGN 8.14)
    const uint64_t tailAt = (rowBytes & ~(uint64_t)15) + lane;
    const bool tail = pBeg + kFlatPiece >= rowBytes && tailAt < rowBytes;
    bool whole[2];
    u32x4 v[2];
    uint8_t b = 0;
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint64_t o = mine + (uint64_t)u * (kFlatPiece / 2);
      whole[u] = o + 16u <= rowBytes;
      v[u] = (u32x4)0u;
      if (whole[u]) v[u] = *(g_cu32x4_a1*)(src + o);
    }
    if (tail) b = *(g_cu8*)(src + tailAt);
    for (uint32_t t = 0; t < n; t++) {
      char* w = (char*)(uintptr_t)flat_alltoall_arg(kOut + 8u * t) + outBase;
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (whole[u]) *(g_u32x4_a1*)(w + mine + u * (kFlatPiece / 2)) = v[u];
      if (tail) *(g_u8*)(w + tailAt) = b;
    }
  }
}

template <int D>
static const void* flat_scatter_v_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&flat_scatter_v_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&flat_scatter_v_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&flat_scatter_v_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&flat_scatter_v_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&flat_scatter_v_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

hipError_t launch_flat_scatter_v(int dt, int op, const FlatScatterVParams& p, unsigned grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (dt) {
    case nexrInt8: fn = flat_scatter_v_fn_dt<nexrInt8>(op); break;
    case nexrUint8: fn = flat_scatter_v_fn_dt<nexrUint8>(op); break;
    case nexrInt32: fn = flat_scatter_v_fn_dt<nexrInt32>(op); break;
    case nexrUint32: fn = flat_scatter_v_fn_dt<nexrUint32>(op); break;
    case nexrInt64: fn = flat_scatter_v_fn_dt<nexrInt64>(op); break;
    case nexrUint64: fn = flat_scatter_v_fn_dt<nexrUint64>(op); break;
    case nexrFloat16: fn = flat_scatter_v_fn_dt<nexrFloat16>(op); break;
    case nexrFloat32: fn = flat_scatter_v_fn_dt<nexrFloat32>(op); break;
    case nexrFloat64: fn = flat_scatter_v_fn_dt<nexrFloat64>(op); break;
    case nexrBfloat16: fn = flat_scatter_v_fn_dt<nexrBfloat16>(op); break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<FlatScatterVParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_gather_v(const FlatScatterVParams& p, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<FlatScatterVParams*>(&p)};
  return hipLaunchKernel((const void*)&flat_gather_v_kernel, dim3(grid), dim3(kBlock), args, 0, s);
}

}  // namespace nexr
