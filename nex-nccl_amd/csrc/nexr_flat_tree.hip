// nexr_flat_tree.hip — the tree all-reduce and the broadcast as ONE launch each with the FIFO collective's own
// bytes (nexrFlatTreeAllReduce, nexrFlatBroadcast), for gfx950. Included at the end of nexr_ll.hip behind
// nexr_flat.hip, whose piece, element accesses and division it shares: the LL / LL128 object stays the one
// code object beside the per-datatype ones.
//
// What it computes. A tree fold is a pure function of an element's position and of its channel's tree
// (runTreeSplit, reference src/device/all_reduce.h:150-230): every rank runs ONE reduce-copy step over its own
// input (through the PreMulSum pre-op) and its children's values in down[] order, a leaf sends a copy of its
// input (a K = 1 step), the root applies the SumPostDiv post-op and its value goes to every output. SIMPLE
// steps fold left from the user input (srcs[0], prims_simple.h:238-242), LL and LL128 steps take every peer as
// the first operand (prims_ll.h:251-258). The host compiles a tree into a program (nexr_api.cpp: LEAF r,
// JOIN r, PUSH, MERGE, one byte each) that consumes every rank's input exactly once; the kernel loads the
// element from the next up to kSymPeers ranks in that order, runs the instructions that consume them in
// registers and goes on. No FIFO, no credit and no poll, so a launch cannot wait for another workgroup.
//
// MI355X mapping, as nexr_flat.hip: a wave takes a piece of 2048 bytes, two 16-byte packs per lane 1024 bytes
// apart. Parts begin at multiples of 16 bytes from element 0, so no pack straddles two parts: a piece that
// holds a part boundary is cut there and each side runs its own tree's program under a lane mask. The program
// counter and the stack pointer are wave-uniform; instructions, the consumption order and the 2n pointers are
// scalar loads from the kernel arguments. The saved accumulators (at most kFlatTreeSlots - 1) stay in VGPRs
// behind wave-uniform compares of the stack pointer with constants, never in a dynamically indexed array
// (DESIGN §8.8 has the numbers against lane-private LDS slots). User pointers are element-aligned only, so
// every pack access is the unaligned-capable form; the buffer's last bytes below a pack go one element per
// lane. Offsets are 64-bit, the cache policy is plain. A lane reads its bytes from every input before it
// stores them, so an output may be an input. A launch covers the byte window [winBeg, winEnd) of the buffer and
// stores out[0 .. nOut), as nexr_flat.hip's: pieces keep their numbers from byte 0, so parts, trees and the tail
// are those of a whole launch.

namespace nexr {

// The saved accumulators of one lane's kPacks positions. `sp` is wave-uniform. One named member per slot, each
// reached through a compare of `sp` with a constant: an array over the slots invites the compiler to fold the
// compares back into one dynamically indexed access, which is scratch. The slots hold a value's 16 bytes as four
// dwords whatever the datatype (a pack of sixteen 8-bit elements would otherwise spread over sixteen registers).
#define NEXR_FLAT_TREE_EACH_SLOT(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)
static_assert(kFlatTreeSlots == 8, "NEXR_FLAT_TREE_EACH_SLOT lists kFlatTreeSlots - 1 slots");
template <int kPacks>
struct FlatTreeSaved {
#define NEXR_FLAT_TREE_MEMBER(i) u32x4 s##i[kPacks];
  NEXR_FLAT_TREE_EACH_SLOT(NEXR_FLAT_TREE_MEMBER)
#undef NEXR_FLAT_TREE_MEMBER
  __device__ __forceinline__ FlatTreeSaved() {
#pragma unroll
    for (int u = 0; u < kPacks; u++) {
#define NEXR_FLAT_TREE_ZERO(i) s##i[u] = (u32x4)0u;
      NEXR_FLAT_TREE_EACH_SLOT(NEXR_FLAT_TREE_ZERO)
#undef NEXR_FLAT_TREE_ZERO
    }
  }
  __device__ __forceinline__ void put(uint32_t sp, const u32x4 (&a)[kPacks]) {
#pragma unroll
    for (int u = 0; u < kPacks; u++) {
#define NEXR_FLAT_TREE_PUT(i) s##i[u] = sp == (uint32_t)i ? a[u] : s##i[u];
      NEXR_FLAT_TREE_EACH_SLOT(NEXR_FLAT_TREE_PUT)
#undef NEXR_FLAT_TREE_PUT
    }
  }
  __device__ __forceinline__ void get(uint32_t sp, u32x4 (&a)[kPacks]) const {
#pragma unroll
    for (int u = 0; u < kPacks; u++) {
#define NEXR_FLAT_TREE_GET(i) a[u] = sp == (uint32_t)i ? s##i[u] : a[u];
      NEXR_FLAT_TREE_EACH_SLOT(NEXR_FLAT_TREE_GET)
#undef NEXR_FLAT_TREE_GET
    }
  }
};

// Byte i of a packed array in the kernel arguments (a scalar dword load and a shift).
__device__ __forceinline__ uint32_t flat_tree_byte(const uint32_t* words, uint32_t i) {
  return (words[i >> 2] >> ((i & 3u) * 8u)) & 0xffu;
}

// Tree t's program over one lane's kPacks positions (kStride bytes apart, from byte `off` of every input): the
// loads of the next up to kSymPeers ranks in consumption order, then the instructions up to the last of their
// consumers. kElem: a position is one element, not a 16-byte pack. A lane whose position is not valid[] loads
// nothing and folds zeros, which it does not store.
template <int D, int OP, bool IsMin, int kPacks, int kStride, bool kElem>
__device__ __forceinline__ void flat_tree_fold(const FlatTreeParams& P, uint32_t t, uint64_t off,
                                               const bool (&valid)[kPacks], u32x4 (&out)[kPacks]) {
  using T = Ty<D>;
  using V = typename T::V;
  constexpr int esz = 16 / T::EPP;
  const FlatTreeProgram& G = P.prog[t];
  const uint32_t nCode = (uint32_t)G.nCode, nIn = (uint32_t)G.nIn;
  const bool userFirst = P.userFirst != 0;
  bool pre = false;
  V factor = bc<V>((u32x4)0u);
  if constexpr (OP == nexrDevPreMulSum) {
    pre = P.preOp != 0;
    factor = T::splat(P.redArg);
  }
  V acc[kPacks];
#pragma unroll
  for (int u = 0; u < kPacks; u++) acc[u] = bc<V>((u32x4)0u);
  FlatTreeSaved<kPacks> saved;
  uint32_t sp = 0, pc = 0;  // wave-uniform, as everything but valid[]
  // PUSH, or MERGE: one more source of the step of the rank whose accumulator was saved
  auto stack_op = [&](uint32_t ins) {
    if ((ins >> 6) == kFlatTreePush) {
      u32x4 bits[kPacks];
#pragma unroll
      for (int u = 0; u < kPacks; u++) bits[u] = bc<u32x4>(acc[u]);
      if (sp < (uint32_t)kFlatTreeSlots - 1) saved.put(sp, bits);
      sp++;
    } else {
      sp = sp ? sp - 1 : 0;
      u32x4 bits[kPacks];
#pragma unroll
      for (int u = 0; u < kPacks; u++) bits[u] = (u32x4)0u;
      saved.get(sp, bits);
#pragma unroll
      for (int u = 0; u < kPacks; u++) {
        const V top = bc<V>(bits[u]);
        const V a = userFirst ? top : acc[u], b = userFirst ? acc[u] : top;
        acc[u] = reduce_step<D, OP, IsMin>(a, b);
        if constexpr (T::kCanon) acc[u] = T::canon(acc[u]);
      }
    }
  };
  for (uint32_t base = 0; base < nIn; base += kSymPeers) {
    u32x4 v[kSymPeers][kPacks];
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nIn) {
        const char* p = P.in[flat_tree_byte(G.order, base + j) & 63u] + off;  // scalar load of the pointer
#pragma unroll
        for (int u = 0; u < kPacks; u++) {
          v[j][u] = (u32x4)0u;
          if (valid[u]) {
            if constexpr (kElem) v[j][u] = flat_ld_elem<esz>(p + u * kStride);
            else v[j][u] = *(g_cu32x4_a1*)(p + u * kStride);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nIn) {
        uint32_t ins = flat_tree_byte(G.code, pc++);
        while ((ins >> 6) >= kFlatTreePush && pc < nCode) {  // what stands before this input's consumer
          stack_op(ins);
          ins = flat_tree_byte(G.code, pc++);
        }
#pragma unroll
        for (int u = 0; u < kPacks; u++) {
          V x = bc<V>(v[j][u]);
          if constexpr (OP == nexrDevPreMulSum) {
            if (pre) x = T::mul(x, factor);  // Apply_PreOp on the rank's own input
          }
          if ((ins >> 6) == kFlatTreeLeaf) {  // the K = 1 step of a leaf: a bit copy without a pre-op
            acc[u] = x;
            if constexpr (T::kCanon && OP == nexrDevPreMulSum) {
              if (pre) acc[u] = T::canon(acc[u]);
            }
          } else {  // JOIN: the rank's own input and its first child's value
            const V a = userFirst ? x : acc[u], b = userFirst ? acc[u] : x;
            acc[u] = reduce_step<D, OP, IsMin>(a, b);
            if constexpr (T::kCanon) acc[u] = T::canon(acc[u]);
          }
        }
      }
    }
  }
  while (pc < nCode) stack_op(flat_tree_byte(G.code, pc++));  // the merges behind the last input
#pragma unroll
  for (int u = 0; u < kPacks; u++) {
    if constexpr (OP == nexrDevSumPostDiv) {
      if (P.postOp) acc[u] = T::divide(acc[u], P.redArg);  // the root's step only
    }
    out[u] = bc<u32x4>(acc[u]);
  }
}

// flat_tree_fold for the launches with a scalar per rank (FlatTreePreMulParams; OP is nexrDevPreMulSum): the same
// program over the same loads, but the pre-op's factor is P.scalars[rank] of the rank whose input the LEAF / JOIN
// consumes, fetched beside that rank's packs as nexr_flat.hip's flat_fold fetches it. A function of its own, so
// that flat_tree_fold and every instance built from it stay as they are.
template <class PT, int D, int kPacks, int kStride, bool kElem>
__device__ __forceinline__ void flat_tree_fold_per_rank(const PT& P, uint32_t t, uint64_t off,
                                                        const bool (&valid)[kPacks], u32x4 (&out)[kPacks]) {
  constexpr int OP = nexrDevPreMulSum;
  using T = Ty<D>;
  using V = typename T::V;
  constexpr int esz = 16 / T::EPP;
  const FlatTreeProgram& G = P.prog[t];
  const uint32_t nCode = (uint32_t)G.nCode, nIn = (uint32_t)G.nIn;
  const bool userFirst = P.userFirst != 0;
  const bool pre = P.preOp != 0;  // 0 under nexrSemanticsShipped only, which launches the plain kernels
  const bool fromMem = pre && P.scalarsArePtrs != 0;
  V factor = bc<V>((u32x4)0u);
  V acc[kPacks];
#pragma unroll
  for (int u = 0; u < kPacks; u++) acc[u] = bc<V>((u32x4)0u);
  FlatTreeSaved<kPacks> saved;
  uint32_t sp = 0, pc = 0;  // wave-uniform, as everything but valid[]
  // PUSH, or MERGE: one more source of the step of the rank whose accumulator was saved
  auto stack_op = [&](uint32_t ins) {
    if ((ins >> 6) == kFlatTreePush) {
      u32x4 bits[kPacks];
#pragma unroll
      for (int u = 0; u < kPacks; u++) bits[u] = bc<u32x4>(acc[u]);
      if (sp < (uint32_t)kFlatTreeSlots - 1) saved.put(sp, bits);
      sp++;
    } else {
      sp = sp ? sp - 1 : 0;
      u32x4 bits[kPacks];
#pragma unroll
      for (int u = 0; u < kPacks; u++) bits[u] = (u32x4)0u;
      saved.get(sp, bits);
#pragma unroll
      for (int u = 0; u < kPacks; u++) {
        const V top = bc<V>(bits[u]);
        const V a = userFirst ? top : acc[u], b = userFirst ? acc[u] : top;
        acc[u] = reduce_step<D, OP, false>(a, b);
        if constexpr (T::kCanon) acc[u] = T::canon(acc[u]);
      }
    }
  };
  for (uint32_t base = 0; base < nIn; base += kSymPeers) {
    u32x4 v[kSymPeers][kPacks];
    FlatScalars<true> sc;  // the scalars of the ranks whose packs are in flight
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nIn) {
        const uint32_t rank = flat_tree_byte(G.order, base + j) & 63u;
        sc.imm[j] = P.scalars[rank];  // by RANK, whatever its place in the program
        sc.lo[j] = sc.hi[j] = 0u;
        if (fromMem) {  // every lane, the same address
          const u32x4 e = flat_ld_elem<esz>((const char*)(uintptr_t)sc.imm[j]);
          sc.lo[j] = e.x;
          if constexpr (esz == 8) sc.hi[j] = e.y;
        }
        const char* p = P.in[rank] + off;  // scalar load of the pointer
#pragma unroll
        for (int u = 0; u < kPacks; u++) {
          v[j][u] = (u32x4)0u;
          if (valid[u]) {
            if constexpr (kElem) v[j][u] = flat_ld_elem<esz>(p + u * kStride);
            else v[j][u] = *(g_cu32x4_a1*)(p + u * kStride);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nIn) {
        uint32_t ins = flat_tree_byte(G.code, pc++);
        while ((ins >> 6) >= kFlatTreePush && pc < nCode) {  // what stands before this input's consumer
          stack_op(ins);
          ins = flat_tree_byte(G.code, pc++);
        }
#pragma unroll
        for (int u = 0; u < kPacks; u++) {
          V x = bc<V>(v[j][u]);
          if (u == 0 && pre) {
            uint64_t bits = sc.imm[j];
            if (fromMem) {
              bits = __builtin_amdgcn_readfirstlane(sc.lo[j]);
              if constexpr (esz == 8) bits |= (uint64_t)__builtin_amdgcn_readfirstlane(sc.hi[j]) << 32;
            }
            factor = T::splat(bits);
          }
          if (pre) x = T::mul(x, factor);  // Apply_PreOp on the rank's own input, by that rank's factor
          if ((ins >> 6) == kFlatTreeLeaf) {  // the K = 1 step of a leaf: a bit copy without a pre-op
            acc[u] = x;
            if constexpr (T::kCanon) {
              if (pre) acc[u] = T::canon(acc[u]);
            }
          } else {  // JOIN: the rank's own input and its first child's value
            const V a = userFirst ? x : acc[u], b = userFirst ? acc[u] : x;
            acc[u] = reduce_step<D, OP, false>(a, b);
            if constexpr (T::kCanon) acc[u] = T::canon(acc[u]);
          }
        }
      }
    }
  }
  while (pc < nCode) stack_op(flat_tree_byte(G.code, pc++));  // the merges behind the last input
#pragma unroll
  for (int u = 0; u < kPacks; u++) out[u] = bc<u32x4>(acc[u]);
}

// The part of element i (wave-uniform): its tree and the element where the part ends.
template <class PT>
__device__ __forceinline__ void flat_tree_part(const PT& P, uint64_t i, uint32_t* t, uint64_t* end) {
  uint32_t lo = 0, hi = (uint32_t)P.nParts - 1;  // the parts tile [0, nElts) in ascending order
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    const uint64_t partEnd = P.ext ? P.ext[mid].offset + P.ext[mid].count : P.parts[mid].offset + P.parts[mid].count;
    if (i < partEnd) hi = mid;
    else lo = mid + 1;
  }
  *t = (P.ext ? P.ext[lo].tree : P.parts[lo].tree) & 1u;
  *end = P.ext ? P.ext[lo].offset + P.ext[lo].count : P.parts[lo].offset + P.parts[lo].count;
}

template <class PT, int D, int OP, bool IsMin>
__device__ __forceinline__ void flat_tree_run(const PT& P) {
  constexpr uint32_t esz = 16 / Ty<D>::EPP;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nOut = (uint32_t)P.nOut;  // the outputs that are stored: the first nOut of out[]
  const uint64_t nBytes = P.nBytes;
  // this launch's pieces: those of the window [winBeg, winEnd), numbered from the buffer's byte 0 (positions are
  // the buffer's, whatever the window); the last one may be short
  const uint64_t winEnd = P.winEnd;
  const uint64_t pieces = (winEnd + kFlatPiece - 1) / kFlatPiece;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = P.winBeg / kFlatPiece + (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < pieces; it += nWaves) {
    const uint64_t pBeg = it * kFlatPiece;
    const uint64_t pEnd = pBeg + kFlatPiece < winEnd ? pBeg + kFlatPiece : winEnd;
    const uint64_t mine = pBeg + lane * 16u;  // this lane's first pack
    uint64_t cur = pBeg;
    while (cur < pEnd) {  // one pass per part that the piece touches: one, but for a piece with a boundary
      uint32_t t;
      uint64_t endElt, end = pEnd;
      flat_tree_part(P, cur / esz, &t, &endElt);
      if (endElt * esz < end) end = endElt * esz;
      {
        bool valid[2];
        u32x4 out[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const uint64_t o = mine + (uint64_t)u * (kFlatPiece / 2);
          valid[u] = o >= cur && o + 16u <= end;  // whole packs of [cur, end)
        }
        if constexpr (PT::kPerRank) flat_tree_fold_per_rank<PT, D, 2, kFlatPiece / 2, false>(P, t, mine, valid, out);
        else flat_tree_fold<D, OP, IsMin, 2, kFlatPiece / 2, false>(P, t, mine, valid, out);
        for (uint32_t r = 0; r < nOut; r++) {
          char* w = P.out[r] + mine;
#pragma unroll
          for (int u = 0; u < 2; u++)
            if (valid[u]) *(g_u32x4_a1*)(w + u * (kFlatPiece / 2)) = out[u];
        }
      }
      const uint32_t tail = (uint32_t)(nBytes & 15u) / esz;
      if (end == nBytes && tail != 0) {  // the buffer's last bytes below a pack: one element per lane
        const uint64_t o = (nBytes & ~(uint64_t)15) + lane * esz;
        bool valid[1] = {lane < tail};
        u32x4 out[1];
        if constexpr (PT::kPerRank) flat_tree_fold_per_rank<PT, D, 1, 0, true>(P, t, o, valid, out);
        else flat_tree_fold<D, OP, IsMin, 1, 0, true>(P, t, o, valid, out);
        for (uint32_t r = 0; r < nOut; r++)
          if (valid[0]) flat_st_elem<esz>(P.out[r] + o, out[0]);
      }
      cur = end;
    }
  }
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void flat_tree_kernel(FlatTreeParams P) {
  if constexpr (OP == nexrDevMinMax) {
    if ((P.redArg & 1) == 0) flat_tree_run<FlatTreeParams, D, OP, true>(P);
    else flat_tree_run<FlatTreeParams, D, OP, false>(P);
  } else {
    flat_tree_run<FlatTreeParams, D, OP, false>(P);
  }
}

// nexrFlatTreeAllReducePreMul: the same run under PreMulSum with a factor per rank, kernels of their own (one per
// datatype) whose argument block trades inline parts for the n scalars.
template <int D>
__global__ __launch_bounds__(kBlock) void flat_tree_premul_kernel(FlatTreePreMulParams P) {
  flat_tree_run<FlatTreePreMulParams, D, nexrDevPreMulSum, false>(P);
}

// Parts beyond the kernel arguments, as flat_parts_kernel.
__global__ __launch_bounds__(kBlock) void flat_tree_parts_kernel(FlatTreePartsFill F) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < (uint32_t)F.n) F.dst[i] = F.parts[i];
}

// The broadcast: nBytes of the root's input to every output that is not the input itself, in the same pieces
// at any byte alignment; the last bytes below a pack go one byte per lane.
__global__ __launch_bounds__(kBlock) void flat_bcast_kernel(FlatBcastParams P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks;
  const uint64_t nBytes = P.nBytes;
  const uint64_t winEnd = P.winEnd;  // the window's pieces, numbered from the buffer's byte 0
  const uint64_t pieces = (winEnd + kFlatPiece - 1) / kFlatPiece;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = P.winBeg / kFlatPiece + (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < pieces; it += nWaves) {
    const uint64_t pBeg = it * kFlatPiece;
    const uint64_t pEnd = pBeg + kFlatPiece < winEnd ? pBeg + kFlatPiece : winEnd;
    const uint64_t mine = pBeg + lane * 16u;
    bool valid[2];
    u32x4 v[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint64_t o = mine + (uint64_t)u * (kFlatPiece / 2);
      valid[u] = o + 16u <= pEnd;
      v[u] = (u32x4)0u;
      if (valid[u]) v[u] = *(g_cu32x4_a1*)(P.in + o);
    }
    const uint32_t tail = (uint32_t)(nBytes & 15u);
    const bool last = pEnd == nBytes && lane < tail;
    const uint64_t to = (nBytes & ~(uint64_t)15) + lane;
    uint8_t b = 0;
    if (last) b = *(g_cu8*)(P.in + to);
    for (uint32_t r = 0; r < n; r++) {
      char* w = P.out[r];
      if (!w) continue;
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (valid[u]) *(g_u32x4_a1*)(w + mine + u * (kFlatPiece / 2)) = v[u];
      if (last) *(g_u8*)(w + to) = b;
    }
  }
}

template <int D>
static const void* flat_tree_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&flat_tree_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&flat_tree_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&flat_tree_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&flat_tree_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&flat_tree_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

static const void* flat_tree_fn(int dt, int op) {
  switch (dt) {
    case nexrInt8: return flat_tree_fn_dt<nexrInt8>(op);
    case nexrUint8: return flat_tree_fn_dt<nexrUint8>(op);
    case nexrInt32: return flat_tree_fn_dt<nexrInt32>(op);
    case nexrUint32: return flat_tree_fn_dt<nexrUint32>(op);
    case nexrInt64: return flat_tree_fn_dt<nexrInt64>(op);
    case nexrUint64: return flat_tree_fn_dt<nexrUint64>(op);
    case nexrFloat16: return flat_tree_fn_dt<nexrFloat16>(op);
    case nexrFloat32: return flat_tree_fn_dt<nexrFloat32>(op);
    case nexrFloat64: return flat_tree_fn_dt<nexrFloat64>(op);
    case nexrBfloat16: return flat_tree_fn_dt<nexrBfloat16>(op);
  }
  return nullptr;
}

hipError_t launch_flat_tree(int dt, int op, const FlatTreeParams& p, unsigned grid, hipStream_t s) {
  const void* fn = flat_tree_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<FlatTreeParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_tree_premul(int dt, const FlatTreePreMulParams& p, unsigned grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (dt) {
    case nexrInt8: fn = (const void*)&flat_tree_premul_kernel<nexrInt8>; break;
    case nexrUint8: fn = (const void*)&flat_tree_premul_kernel<nexrUint8>; break;
    case nexrInt32: fn = (const void*)&flat_tree_premul_kernel<nexrInt32>; break;
    case nexrUint32: fn = (const void*)&flat_tree_premul_kernel<nexrUint32>; break;
    case nexrInt64: fn = (const void*)&flat_tree_premul_kernel<nexrInt64>; break;
    case nexrUint64: fn = (const void*)&flat_tree_premul_kernel<nexrUint64>; break;
    case nexrFloat16: fn = (const void*)&flat_tree_premul_kernel<nexrFloat16>; break;
    case nexrFloat32: fn = (const void*)&flat_tree_premul_kernel<nexrFloat32>; break;
    case nexrFloat64: fn = (const void*)&flat_tree_premul_kernel<nexrFloat64>; break;
    case nexrBfloat16: fn = (const void*)&flat_tree_premul_kernel<nexrBfloat16>; break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<FlatTreePreMulParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_tree_parts(const FlatTreePartsFill& f, hipStream_t s) {
  void* args[] = {const_cast<FlatTreePartsFill*>(&f)};
  return hipLaunchKernel((const void*)&flat_tree_parts_kernel, dim3((unsigned)((f.n + kBlock - 1) / kBlock)),
                         dim3(kBlock), args, 0, s);
}

hipError_t launch_flat_bcast(const FlatBcastParams& p, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<FlatBcastParams*>(&p)};
  return hipLaunchKernel((const void*)&flat_bcast_kernel, dim3(grid), dim3(kBlock), args, 0, s);
}

}  // namespace nexr
