// nexr_flat_group.hip — SEVERAL flat collectives in one launch (nexrFlatGroup), for gfx950. Included at the end
// of nexr_ll.hip behind nexr_flat_tree.hip: the LL / LL128 object stays the one code object beside the
// per-datatype ones.
//
// What it computes. A launch runs a TABLE of works of one (datatype, device op, min-or-max): each a ring
// all-reduce, reduce-scatter or reduce with its own buffers, element count, root, redOpArg and channel parts,
// every one by flat_run / flat_fold of nexr_flat.hip, the code of the single calls: the per-element rule, the
// pieces, the cut at a chunk boundary, the sub-pack tail, the operand order and the semantics are not restated
// here. The launch's items are the concatenation of every work's pieces (times its regions for a
// reduce-scatter); itemEnd of a record is the prefix sum up to and including its work.
//
// How a wave finds its work. The item number is wave-uniform, so the binary search over the records' itemEnd
// and every read of the record found are scalar loads through the constant address space: of the kernel
// arguments where the table rides there, of the call's stream-ordered workspace where it does not (filled by
// flat_group_fill_kernel launches ahead of this one in the same stream). Everything but valid[] stays
// wave-uniform, as in flat_run. The partition is static: no atomics, no polls, no LDS, and a capped grid strides
// over the items, so a launch cannot wait on residency.
//
// The table (nexr_internal.h): nWorks records of kFlatGroupRecBytes + 16 * nRanks bytes, {itemEnd, regionBytes,
// redArg, coll, root, nParts, partsAt, in[nRanks], out[nRanks]}, then the pool of every all-reduce's parts.
// flat_group_copy_kernel: records of kFlatGroupCopyRecBytes + 8 * maxOut bytes, {itemEnd, nBytes, src,
// dst[maxOut]}; a null destination or one at the source's address is not written.

namespace nexr {

typedef __attribute__((address_space(4))) const char c_tbl;
template <class T>
__device__ __forceinline__ T tbl_ld(c_tbl* p) {
  return *(__attribute__((address_space(4))) const T*)p;
}

// The table of a launch: the workspace, or the bytes behind the header in the kernel arguments.
template <class GP>
__device__ __forceinline__ c_tbl* flat_group_table(const GP& G) {
  c_tbl* inl = (c_tbl*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(GP, inl);
  return G.ext ? (c_tbl*)(uintptr_t)G.ext : inl;
}

// The record of item `it` (wave-uniform): the first whose itemEnd is above it; *local its number inside the work.
__device__ __forceinline__ c_tbl* flat_group_find(c_tbl* tbl, uint32_t nWorks, uint32_t stride, uint64_t it,
                                                  uint64_t* local) {
  uint32_t lo = 0, hi = nWorks - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (it < tbl_ld<uint64_t>(tbl + (uint64_t)mid * stride)) hi = mid;
    else lo = mid + 1;
  }
  c_tbl* rec = tbl + (uint64_t)lo * stride;
  *local = it - (lo ? tbl_ld<uint64_t>(rec - stride) : 0);
  return rec;
}

// One item of one work as flat_run / flat_fold / flat_chunk read a launch's parameters (FlatParams' names, kOneItem:
// flat_run does the wave's one item): the launch's fields by value, the work's pointers and parts as scalar loads
// of its record.
struct FlatGroupView {
  static constexpr bool kPerRank = false;
  static constexpr bool kOneItem = true;
  static constexpr const nexrFlatPart* ext = nullptr;  // the parts are parts[]
  static constexpr uint64_t winBeg = 0;                // the whole region
  struct In {
    c_tbl* at;
    __device__ __forceinline__ const char* operator[](uint32_t r) const {
      return (const char*)(uintptr_t)tbl_ld<uint64_t>(at + 8u * r);
    }
  } in;
  struct Out {
    c_tbl* at;
    __device__ __forceinline__ char* operator[](uint32_t r) const {
      return (char*)(uintptr_t)tbl_ld<uint64_t>(at + 8u * r);
    }
  } out;
  struct Parts {
    c_tbl* at;
    __device__ __forceinline__ nexrFlatPart operator[](uint32_t k) const {
      c_tbl* p = at + (uint64_t)k * sizeof(nexrFlatPart);
      return nexrFlatPart{tbl_ld<uint64_t>(p), tbl_ld<uint64_t>(p + 8), tbl_ld<uint64_t>(p + 16)};
    }
  } parts;
  uint64_t item;  // the item inside the work
  uint64_t regionBytes, winEnd, redArg;
  int coll, nRanks, nFold, shift, userFirst, preOp, postOp, root, nParts, nOut;
};

template <int D, int OP, bool IsMin>
__device__ __forceinline__ void flat_group_run(const FlatGroupParams& G) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)G.nRanks;
  const uint32_t stride = kFlatGroupRecBytes + 16u * n;
  c_tbl* tbl = flat_group_table(G);
  const uint64_t nItems = G.nItems;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
    FlatGroupView V;
    c_tbl* rec = flat_group_find(tbl, (uint32_t)G.nWorks, stride, it, &V.item);
    V.in.at = rec + kFlatGroupRecBytes;
    V.out.at = rec + kFlatGroupRecBytes + 8u * n;
    V.parts.at = tbl + G.poolAt + (uint64_t)tbl_ld<uint32_t>(rec + 36) * sizeof(nexrFlatPart);
    V.regionBytes = V.winEnd = tbl_ld<uint64_t>(rec + 8);
    V.redArg = tbl_ld<uint64_t>(rec + 16);
    V.coll = (int)tbl_ld<uint32_t>(rec + 24);
    V.root = (int)tbl_ld<uint32_t>(rec + 28);
    V.nParts = (int)tbl_ld<uint32_t>(rec + 32);
    V.nRanks = V.nOut = (int)n;
    V.nFold = G.nFold;
    V.shift = G.shift;
    V.userFirst = G.userFirst;
    V.preOp = G.preOp;
    V.postOp = G.postOp;
    flat_run<FlatGroupView, D, OP, IsMin>(V);  // the single calls' code on that one item
  }
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void flat_group_kernel(FlatGroupParams G) {
  if constexpr (OP == nexrDevMinMax) {
    if (G.isMin) flat_group_run<D, OP, true>(G);  // one value per launch: the host splits on it
    else flat_group_run<D, OP, false>(G);
  } else {
    flat_group_run<D, OP, false>(G);
  }
}

// Copies (a broadcast is one work, an all-gather n): flat_bcast_kernel's piece for the work of the item.
__global__ __launch_bounds__(kBlock) void flat_group_copy_kernel(FlatGroupCopyParams G) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t maxOut = (uint32_t)G.maxOut;
  const uint32_t stride = kFlatGroupCopyRecBytes + 8u * maxOut;
  c_tbl* tbl = flat_group_table(G);
  const uint64_t nItems = G.nItems;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
    uint64_t local;
    c_tbl* rec = flat_group_find(tbl, (uint32_t)G.nWorks, stride, it, &local);
    const uint64_t nBytes = tbl_ld<uint64_t>(rec + 8);
    const char* src = (const char*)(uintptr_t)tbl_ld<uint64_t>(rec + 16);
    const uint64_t pBeg = local * kFlatPiece;
    const uint64_t pEnd = pBeg + kFlatPiece < nBytes ? pBeg + kFlatPiece : nBytes;
    const uint64_t mine = pBeg + lane * 16u;
    bool valid[2];
    u32x4 v[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint64_t o = mine + (uint64_t)u * (kFlatPiece / 2);
      valid[u] = o + 16u <= pEnd;
      v[u] = (u32x4)0u;
      if (valid[u]) v[u] = *(g_cu32x4_a1*)(src + o);
    }
    const uint32_t tail = (uint32_t)(nBytes & 15u);
    const bool last = pEnd == nBytes && lane < tail;
    const uint64_t to = (nBytes & ~(uint64_t)15) + lane;
    uint8_t b = 0;
    if (last) b = *(g_cu8*)(src + to);
    for (uint32_t r = 0; r < maxOut; r++) {
      char* w = (char*)(uintptr_t)tbl_ld<uint64_t>(rec + kFlatGroupCopyRecBytes + 8u * r);
      if (!w || w == src) continue;
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (valid[u]) *(g_u32x4_a1*)(w + mine + u * (kFlatPiece / 2)) = v[u];
      if (last) *(g_u8*)(w + to) = b;
    }
  }
}

// A table beyond the kernel arguments: a launch of this copies up to kFlatGroupFillWords of its 8-byte words,
// passed by value, into the call's stream-ordered workspace.
__global__ __launch_bounds__(kBlock) void flat_group_fill_kernel(FlatGroupFill F) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < (uint32_t)F.n) F.dst[i] = F.words[i];
}

template <int D>
static const void* flat_group_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&flat_group_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&flat_group_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&flat_group_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&flat_group_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&flat_group_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

hipError_t launch_flat_group(int dt, int op, const FlatGroupParams& p, unsigned grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (dt) {
    case nexrInt8: fn = flat_group_fn_dt<nexrInt8>(op); break;
    case nexrUint8: fn = flat_group_fn_dt<nexrUint8>(op); break;
    case nexrInt32: fn = flat_group_fn_dt<nexrInt32>(op); break;
    case nexrUint32: fn = flat_group_fn_dt<nexrUint32>(op); break;
    case nexrInt64: fn = flat_group_fn_dt<nexrInt64>(op); break;
    case nexrUint64: fn = flat_group_fn_dt<nexrUint64>(op); break;
    case nexrFloat16: fn = flat_group_fn_dt<nexrFloat16>(op); break;
    case nexrFloat32: fn = flat_group_fn_dt<nexrFloat32>(op); break;
    case nexrFloat64: fn = flat_group_fn_dt<nexrFloat64>(op); break;
    case nexrBfloat16: fn = flat_group_fn_dt<nexrBfloat16>(op); break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<FlatGroupParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_group_copy(const FlatGroupCopyParams& p, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<FlatGroupCopyParams*>(&p)};
  return hipLaunchKernel((const void*)&flat_group_copy_kernel, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_group_fill(const FlatGroupFill& f, hipStream_t s) {
  void* args[] = {const_cast<FlatGroupFill*>(&f)};
  return hipLaunchKernel((const void*)&flat_group_fill_kernel, dim3((unsigned)((f.n + kBlock - 1) / kBlock)),
                         dim3(kBlock), args, 0, s);
}

}  // namespace nexr
