// nexr_flat.hip — the ring all-reduce, reduce-scatter and reduce as ONE launch with the ring's own bytes
// (nexrFlatAllReduce, nexrFlatReduceScatter, nexrFlatReduce), for gfx950. Included at the end of nexr_ll.hip
// behind nexr_sym.hip, whose access types and kSymPeers it shares: the LL / LL128 object stays the one code
// object beside the per-datatype ones.
//
// What it computes. A ring fold is a pure function of an element's position (runRing, reference
// src/device/all_reduce.h:12-84, reduce_scatter.h:12-52, reduce.h:12-50): the chain starts at rank s with a
// copy of in[s] (directSend / sendInput: a K = 1 step, with the PreMulSum pre-op and then that step's
// ncclFromFloat canonicalisation), and every following rank r = s + 1, ..., s + n - 1 (mod n) runs ONE
// reduce-copy step over {its own input through the pre-op, the partial}, with its own rounding and its own
// fp16 / bf16 NaN canonicalisation; the last one applies the SumPostDiv post-op. SIMPLE steps take the user
// input as first operand (srcs[0], prims_simple.h:238-242; simple_fold, nexrReduceCopy), LL and LL128 steps
// the partial (prims_ll.h:251-258, prims_ll128.h:214-219). The kernel loads the element from every rank's
// input, runs that chain in registers and stores the result: no FIFO, no credit and no poll, so a launch
// cannot wait for another workgroup. Which rank a chain starts at is include/nexr.h's rule: the
// reduce-scatter's chunk d at d + 1, the reduce at root + 1, the all-reduce's element by the chunk of its
// channel part's loop (flat_chunk below restates runRingAllReduce, nexr_ring.cpp).
//
// MI355X mapping, as nexr_sym.hip: a wave takes a piece of 2048 bytes of a region (the all-reduce's or the
// reduce's buffer, one chunk of the reduce-scatter), two 16-byte packs per lane 1024 bytes apart. Every chunk
// boundary of the all-reduce lies a multiple of 16 bytes from element 0 (cells, grains and the last loop's
// alignment), so no pack straddles two chunks: a piece that holds a boundary is cut there and each side runs
// with its own start rank under a lane mask. The start rank is therefore wave-uniform and the 2n pointers are
// scalar loads from the kernel arguments. Up to kSymPeers ranks' packs are loaded before the first fold step;
// beyond that the chain goes on in groups of kSymPeers. User pointers are element-aligned only (a chunk's
// phase differs by rank), so every pack access is the unaligned-capable form; the region's last bytes below a
// pack go one element per lane. Offsets are 64-bit. No LDS, no cross-lane traffic, plain cache policy. A lane
// reads its bytes from every input before it stores them, so an output may be an input.
//
// The window. A launch covers the bytes [winBeg, winEnd) of every region (winBeg a multiple of the piece; 0 and
// regionBytes: the whole region, the device entries' launch). Only the enumeration of the pieces knows it: a
// piece keeps its number from the region's byte 0, so a position, its chunk, its start rank and the sub-pack tail
// at the region's end are what they are in a whole launch, and `pointer + region offset` addresses every buffer
// (the host entries pass a staged window's buffer biased by -winBeg, nexr_api.cpp). The all-reduce stores the
// first nOut entries of out[] (n, or fewer where outputs share a staged buffer). Both are wave-uniform kernel
// arguments: no instance's VGPRs, scratch or occupancy changed with them (docs/HISTORY.md, round 19).

namespace nexr {

constexpr int kFlatPiece = 2048;
typedef __attribute__((address_space(1))) const uint64_t g_cu64;
typedef __attribute__((address_space(1))) uint64_t g_u64;

// One element at an element-aligned address as the low bytes of a zero pack, and back.
template <int ESZ>
__device__ __forceinline__ u32x4 flat_ld_elem(const char* p) {
  u32x4 v = (u32x4)0u;
  if constexpr (ESZ == 1) v.x = *(g_cu8*)p;
  else if constexpr (ESZ == 2) v.x = *(g_cu16*)p;
  else if constexpr (ESZ == 4) v.x = *(g_cu32*)p;
  else {
    const uint64_t x = *(g_cu64*)p;
    v.x = (uint32_t)x;
    v.y = (uint32_t)(x >> 32);
  }
  return v;
}
template <int ESZ>
__device__ __forceinline__ void flat_st_elem(char* p, u32x4 v) {
  if constexpr (ESZ == 1) *(g_u8*)p = (uint8_t)v.x;
  else if constexpr (ESZ == 2) *(g_u16*)p = (uint16_t)v.x;
  else if constexpr (ESZ == 4) *(g_u32*)p = v.x;
  else *(g_u64*)p = (uint64_t)v.y << 32 | v.x;
}

// a / b for wave-uniform operands: the 32-bit division whenever both fit
__device__ __forceinline__ uint64_t flat_div(uint64_t a, uint64_t b) {
  return ((a | b) >> 32) ? a / b : (uint64_t)((uint32_t)a / (uint32_t)b);
}

// With a scalar per rank: the scalar of each rank in flight, imm its bits or where they are, lo / hi the element
// loaded from there (hi: 8-byte types). Nothing at all in the launches with one factor.
template <bool kPerRank>
struct FlatScalars {};
template <>
struct FlatScalars<true> {
  uint64_t imm[kSymPeers];
  uint32_t lo[kSymPeers], hi[kSymPeers];
};
template <class PT>
__device__ __forceinline__ bool flat_scalars_from_mem(const PT& P, bool pre) {
  if constexpr (PT::kPerRank) return pre && P.scalarsArePtrs != 0;
  else return false;
}

// The chain of one lane's kPacks positions (kStride bytes apart, from byte `off` of every input), started at
// rank `first`: the loads of up to kSymPeers ranks, then their steps. kElem: a position is one element, not
// a 16-byte pack. A lane whose position is not valid[] loads nothing and folds zeros, which it does not store.
// PT: the launch's parameters. With PT::kPerRank (FlatPreMulParams: a user-created PreMulSum op) the pre-op's
// factor is the one of the RANK whose packs are being loaded, P.scalars[r], not one factor for the chain: it is
// fetched in the load phase beside that rank's packs, a scalar load of the kernel argument for an immediate, or,
// for a device-resident scalar (element-aligned only), one load of the element at a wave-uniform address by
// every lane, made a scalar by readfirstlane where the step multiplies. The kernel reads such a scalar itself:
// whatever the stream wrote before the launch is what it sees.
template <class PT, int D, int OP, bool IsMin, int kPacks, int kStride, bool kElem>
__device__ __forceinline__ void flat_fold(const PT& P, uint32_t first, uint64_t off,
                                          const bool (&valid)[kPacks], u32x4 (&out)[kPacks]) {
  using T = Ty<D>;
  using V = typename T::V;
  constexpr int esz = 16 / T::EPP;
  const uint32_t n = (uint32_t)P.nRanks, nFold = (uint32_t)P.nFold;
  const bool userFirst = P.userFirst != 0;
  bool pre = false;
  V factor = bc<V>((u32x4)0u);
  if constexpr (OP == nexrDevPreMulSum) {
    pre = P.preOp != 0;
    if constexpr (!PT::kPerRank) factor = T::splat(P.redArg);
  }
  const bool fromMem = flat_scalars_from_mem(P, pre);
  V acc[kPacks];
  uint32_t r = first;
  for (uint32_t base = 0; base < nFold; base += kSymPeers) {  // wave-uniform, as everything but valid[]
    u32x4 v[kSymPeers][kPacks];
    FlatScalars<PT::kPerRank> sc;  // PT::kPerRank: the scalars of the ranks whose packs are in flight
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nFold) {
        if constexpr (PT::kPerRank) {
          sc.imm[j] = P.scalars[r];
          sc.lo[j] = sc.hi[j] = 0u;
          if (fromMem) {  // every lane, the same address
            const u32x4 e = flat_ld_elem<esz>((const char*)(uintptr_t)sc.imm[j]);
            sc.lo[j] = e.x;
            if constexpr (esz == 8) sc.hi[j] = e.y;
          }
        }
        const char* p = P.in[r] + off;  // scalar load of the pointer
#pragma unroll
        for (int u = 0; u < kPacks; u++) {
          v[j][u] = (u32x4)0u;
          if (valid[u]) {
            if constexpr (kElem) v[j][u] = flat_ld_elem<esz>(p + u * kStride);
            else v[j][u] = *(g_cu32x4_a1*)(p + u * kStride);
          }
        }
        r = r + 1 == n ? 0 : r + 1;
      }
    }
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nFold) {
#pragma unroll
        for (int u = 0; u < kPacks; u++) {
          V x = bc<V>(v[j][u]);
          if constexpr (PT::kPerRank) {
            if (u == 0 && pre) {
              uint64_t bits = sc.imm[j];
              if (fromMem) {
                bits = __builtin_amdgcn_readfirstlane(sc.lo[j]);
                if constexpr (esz == 8) bits |= (uint64_t)__builtin_amdgcn_readfirstlane(sc.hi[j]) << 32;
              }
              factor = T::splat(bits);
            }
          }
          if constexpr (OP == nexrDevPreMulSum) {
            if (pre) x = T::mul(x, factor);  // Apply_PreOp on the rank's own input
          }
          if (j == 0 && base == 0) {  // the K = 1 step of the chain's first rank: a bit copy without a pre-op
            acc[u] = x;
            if constexpr (T::kCanon && OP == nexrDevPreMulSum) {
              if (pre) acc[u] = T::canon(acc[u]);
            }
          } else {  // one reduce-copy step of {the rank's input, the partial}, and its canonicalisation
            const V a = userFirst ? x : acc[u], b = userFirst ? acc[u] : x;
            acc[u] = reduce_step<D, OP, IsMin>(a, b);
            if constexpr (T::kCanon) acc[u] = T::canon(acc[u]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kPacks; u++) {
    if constexpr (OP == nexrDevSumPostDiv) {
      if (P.postOp) acc[u] = T::divide(acc[u], P.redArg);  // the chain's last step only
    }
    out[u] = bc<u32x4>(acc[u]);
  }
}

// The all-reduce's chunk of element i (wave-uniform): the start rank of its chain and the element where the
// chunk ends. runRingAllReduce (nexr_ring.cpp; all_reduce.h:12-84) for the part {offset, count, chunkCount}
// that holds i: loops of n * chunkCount elements, the last one in chunks of alignUp(divUp(rem, n), 16 / esz),
// chunk c of a loop started by rank c + 1.
template <class PT>
__device__ __forceinline__ void flat_chunk(const PT& P, uint64_t i, uint32_t epp, uint32_t* s, uint64_t* end) {
  const uint32_t n = (uint32_t)P.nRanks;
  uint32_t lo = 0, hi = (uint32_t)P.nParts - 1;  // the parts tile [0, nElts) in ascending order
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    const uint64_t partEnd = P.ext ? P.ext[mid].offset + P.ext[mid].count : P.parts[mid].offset + P.parts[mid].count;
    if (i < partEnd) hi = mid;
    else lo = mid + 1;
  }
  const uint64_t offset = P.ext ? P.ext[lo].offset : P.parts[lo].offset;
  const uint64_t count = P.ext ? P.ext[lo].count : P.parts[lo].count;
  const uint64_t chunkCount = P.ext ? P.ext[lo].chunkCount : P.parts[lo].chunkCount;
  const uint64_t j = i - offset, loop = (uint64_t)n * chunkCount;
  const uint64_t L = flat_div(j, loop);
  const uint64_t rem = count - L * loop, jj = j - L * loop;
  uint64_t cc = chunkCount;
  if (rem < loop) cc = flat_div(flat_div(rem + n - 1, n) + epp - 1, epp) * epp;
  const uint64_t c = flat_div(jj, cc);
  const uint64_t chunkEnd = (c + 1) * cc;
  *s = (uint32_t)c + 1 == n ? 0 : (uint32_t)c + 1;
  *end = offset + L * loop + (chunkEnd < rem ? chunkEnd : rem);
}

template <class PT, int D, int OP, bool IsMin>
__device__ __forceinline__ void flat_run(const PT& P) {
  constexpr uint32_t esz = 16 / Ty<D>::EPP;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks, coll = (uint32_t)P.coll;
  const uint32_t nRegions = coll == kFlatReduceScatter ? n : 1u;
  const uint64_t regBytes = P.regionBytes;
  // this launch's pieces of every region: those of the window [winBeg, winEnd), numbered from the region's byte
  // 0 (positions are the region's, whatever the window); the last one may be short
  const uint64_t winEnd = P.winEnd, piece0 = P.winBeg / kFlatPiece;
  const uint64_t pieces = (winEnd + kFlatPiece - 1) / kFlatPiece - piece0;
  const uint64_t nItems = pieces * nRegions;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  const uint32_t shift = (uint32_t)P.shift;
  const uint32_t nOut = coll == kFlatAllReduce ? (uint32_t)P.nOut : 1u;
  uint64_t it0 = (uint64_t)blockIdx.x * (kBlock / 64) + wave, itEnd = nItems;
  if constexpr (PT::kOneItem) {  // flat_group_run (nexr_flat_group.hip): the wave's one item of the work P views
    it0 = P.item;
    itEnd = P.item + 1;
  }
  for (uint64_t it = it0; it < itEnd; it += nWaves) {
    uint64_t k = it;
    uint32_t d = 0;
    if (nRegions > 1) sym_split(it, nRegions, &k, &d);  // region fastest: few waves still touch every chunk
    const uint64_t pBeg = (piece0 + k) * kFlatPiece;
    const uint64_t pEnd = pBeg + kFlatPiece < winEnd ? pBeg + kFlatPiece : winEnd;
    const uint64_t inBase = (uint64_t)d * regBytes;  // chunk d of every input
    const uint64_t mine = pBeg + lane * 16u;         // this lane's first pack, from the region's byte 0
    uint64_t cur = pBeg;
    while (cur < pEnd) {  // one pass per chunk that the piece touches: one, but for a piece with a boundary
      uint32_t s;
      uint64_t end = pEnd;
      if (coll == kFlatAllReduce) {
        uint64_t endElt;
        flat_chunk(P, cur / esz, 16u / esz, &s, &endElt);
        if (endElt * esz < end) end = endElt * esz;
      } else {
        s = coll == kFlatReduceScatter ? d + 1 : (uint32_t)P.root + 1;
        s = s == n ? 0 : s;
      }
      uint32_t first = s + shift;  // the rank whose input starts what is folded (s but under shipped semantics)
      first = first >= n ? first - n : first;
      const uint32_t outFirst = coll == kFlatAllReduce ? 0u : coll == kFlatReduceScatter ? d : (uint32_t)P.root;
      {
        bool valid[2];
        u32x4 out[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const uint64_t o = mine + (uint64_t)u * (kFlatPiece / 2);
          valid[u] = o >= cur && o + 16u <= end;  // whole packs of [cur, end)
        }
        flat_fold<PT, D, OP, IsMin, 2, kFlatPiece / 2, false>(P, first, inBase + mine, valid, out);
        uint32_t r = outFirst;
        for (uint32_t q = 0; q < nOut; q++) {
          char* w = P.out[r] + mine;
#pragma unroll
          for (int u = 0; u < 2; u++)
            if (valid[u]) *(g_u32x4_a1*)(w + u * (kFlatPiece / 2)) = out[u];
          r++;
        }
      }
      const uint32_t tail = (uint32_t)(regBytes & 15u) / esz;
      if (end == regBytes && tail != 0) {  // the region's last bytes below a pack: one element per lane
        const uint64_t o = (regBytes & ~(uint64_t)15) + lane * esz;
        bool valid[1] = {lane < tail};
        u32x4 out[1];
        flat_fold<PT, D, OP, IsMin, 1, 0, true>(P, first, inBase + o, valid, out);
        uint32_t r = outFirst;
        for (uint32_t q = 0; q < nOut; q++) {
          if (valid[0]) flat_st_elem<esz>(P.out[r] + o, out[0]);
          r++;
        }
      }
      cur = end;
    }
  }
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void flat_kernel(FlatParams P) {
  if constexpr (OP == nexrDevMinMax) {
    if ((P.redArg & 1) == 0) flat_run<FlatParams, D, OP, true>(P);
    else flat_run<FlatParams, D, OP, false>(P);
  } else {
    flat_run<FlatParams, D, OP, false>(P);
  }
}

// nexrFlatAllReducePreMul, nexrFlatReduceScatterPreMul, nexrFlatReducePreMul: the same run under PreMulSum with a
// factor per rank (flat_fold's PT::kPerRank). Kernels of their own, one per datatype: the instances above are at
// their SGPR limit and stay as they are.
template <int D>
__global__ __launch_bounds__(kBlock) void flat_premul_kernel(FlatPreMulParams P) {
  flat_run<FlatPreMulParams, D, nexrDevPreMulSum, false>(P);
}

// Parts beyond the kernel arguments: a launch of this copies up to kFlatInlineParts of them, passed by value,
// into the call's stream-ordered workspace.
__global__ __launch_bounds__(kBlock) void flat_parts_kernel(FlatPartsFill F) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < (uint32_t)F.n) F.dst[i] = F.parts[i];
}

template <int D>
static const void* flat_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&flat_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&flat_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&flat_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&flat_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&flat_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

static const void* flat_fn(int dt, int op) {
  switch (dt) {
    case nexrInt8: return flat_fn_dt<nexrInt8>(op);
    case nexrUint8: return flat_fn_dt<nexrUint8>(op);
    case nexrInt32: return flat_fn_dt<nexrInt32>(op);
    case nexrUint32: return flat_fn_dt<nexrUint32>(op);
    case nexrInt64: return flat_fn_dt<nexrInt64>(op);
    case nexrUint64: return flat_fn_dt<nexrUint64>(op);
    case nexrFloat16: return flat_fn_dt<nexrFloat16>(op);
    case nexrFloat32: return flat_fn_dt<nexrFloat32>(op);
    case nexrFloat64: return flat_fn_dt<nexrFloat64>(op);
    case nexrBfloat16: return flat_fn_dt<nexrBfloat16>(op);
  }
  return nullptr;
}

hipError_t launch_flat(int dt, int op, const FlatParams& p, unsigned grid, hipStream_t s) {
  const void* fn = flat_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<FlatParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_premul(int dt, const FlatPreMulParams& p, unsigned grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (dt) {
    case nexrInt8: fn = (const void*)&flat_premul_kernel<nexrInt8>; break;
    case nexrUint8: fn = (const void*)&flat_premul_kernel<nexrUint8>; break;
    case nexrInt32: fn = (const void*)&flat_premul_kernel<nexrInt32>; break;
    case nexrUint32: fn = (const void*)&flat_premul_kernel<nexrUint32>; break;
    case nexrInt64: fn = (const void*)&flat_premul_kernel<nexrInt64>; break;
    case nexrUint64: fn = (const void*)&flat_premul_kernel<nexrUint64>; break;
    case nexrFloat16: fn = (const void*)&flat_premul_kernel<nexrFloat16>; break;
    case nexrFloat32: fn = (const void*)&flat_premul_kernel<nexrFloat32>; break;
    case nexrFloat64: fn = (const void*)&flat_premul_kernel<nexrFloat64>; break;
    case nexrBfloat16: fn = (const void*)&flat_premul_kernel<nexrBfloat16>; break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<FlatPreMulParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_parts(const FlatPartsFill& f, hipStream_t s) {
  void* args[] = {const_cast<FlatPartsFill*>(&f)};
  return hipLaunchKernel((const void*)&flat_parts_kernel, dim3((unsigned)((f.n + kBlock - 1) / kBlock)), dim3(kBlock),
                         args, 0, s);
}

}  // namespace nexr
