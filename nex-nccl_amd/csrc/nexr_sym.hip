// nexr_sym.hip — the symmetric all-reduce RSxLD_AGxST as ONE launch (nexrSymAllReduce), for gfx950, and behind
// it its siblings ReduceScatter_LD and AllGather_ST (nexrSymReduceScatter, nexrSymAllGather; their own comment
// below) and the family's LL members AllReduce_AGxLL_R, ReduceScatter_LL and AllGather_LL (nexrSymLL*; at the end
// of the file). Included at the end of nexr_ll.hip behind nexr_simple.hip: the LL / LL128 object stays the one code
// object beside the per-datatype ones.
//
// What it computes is ncclSymRun_AllReduce_RSxLD_AGxST (reference src/device/symmetric/all_reduce.hh:6-276)
// on a communicator whose ranks all live on this GPU: every "peer window" is a plain device buffer, and the
// cross-rank barriers at both ends of the reference kernel (:269-275) are the stream's order. Each rank owns
// every n-th piece of the buffer; the owner o of an element loads it from every rank's input, folds
// acc = in[o]; acc = acc + in[(o + j) % n], j = 1..n-1 (allreduceDeep :23-81, allreduceEnds :134-169), in
// fp32 for all three datatypes (ncclSymAccumType, symmetric/primitives.hh:426-434; fp16 / bf16 widened
// exactly, ONE round-to-nearest-even back, every NaN to 0x7fff), and stores the result to every rank's
// output (:83-104, :171-188). Which bytes are which rank's is planned on the host (symPlan, nexr_api.cpp)
// from rank 0's pointers as the reference does (:199-252) and arrives as SymParams:
//   pass 1   p1Pieces pieces of 2048 bytes from byte p1Off, piece i owned by rank i % n (16-byte packs);
//   pass 2   p2Pieces pieces of 512 bytes from byte p2Off, piece i owned by rank i % n (4-byte packs);
//   ends     nEnds elements: the preElts leading ones, then those from byte sufOff; element e owned by rank
//            (e / 32) % n, one element per lane.
// The reference reaches this map with warps of 32 numbered rank, block, warp (:262-267): a warp's iteration
// is 4 packs x 32 lanes, and warp w takes iterations w, w + wn, ... with n | wn.
//
// MI355X mapping. A wave takes whole pieces, so the owner is wave-uniform and the 2n pointers are scalar
// loads from the kernel arguments: no lane holds a pointer per rank. A 2048-byte piece is two 16-byte packs
// per lane of a wave64, a 512-byte piece two 4-byte packs, a group of 32 end elements the wave's low half.
// All the loads of a wave's piece, for up to kSymPeers peers, are issued before the first add; beyond
// kSymPeers ranks the fold goes on in groups of kSymPeers so that the registers stay bounded. Rank 0's
// buffers decide the passes (its pass-1 packs are 16-byte aligned, its pass-2 packs 4-byte aligned); the
// other ranks' buffers may sit at any element-aligned address, so every pack access is the unaligned-capable
// form (nexr_types.hpp). No LDS, no cross-lane traffic, plain cache policy, a one-shot grid over the pieces.
// An element is read by its one owner before anybody writes it, so any output may be any input.

namespace nexr {

constexpr int kSymPeers = 8;         // peers whose packs a wave has in flight at once
constexpr int kSymPiece16 = 2048;    // pass 1: 4 packs x 32 lanes x 16 bytes of the reference
constexpr int kSymPiece4 = 512;      // pass 2: 4 packs x 32 lanes x 4 bytes
constexpr int kSymEndGroup = 32;     // ends: the reference's warp

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// a 4-byte pack of two 16-bit elements at any 2-byte aligned address
typedef uint32_t __attribute__((aligned(1))) u32_a1;
typedef __attribute__((address_space(1))) const u32_a1 g_cu32_a1;
typedef __attribute__((address_space(1))) u32_a1 g_u32_a1;
typedef __attribute__((address_space(1))) const uint16_t g_cu16;
typedef __attribute__((address_space(1))) uint16_t g_u16;
typedef __attribute__((address_space(1))) const uint32_t g_cu32;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) const uint8_t g_cu8;
typedef __attribute__((address_space(1))) uint8_t g_u8;

// ncclFromFloat's NaN (0x7fff) for a vector of fp16 / bf16 bit patterns; infBits = 0x7c00 / 0x7f80
template <typename UV>
__device__ __forceinline__ UV sym_canon(UV x, uint16_t infBits) {
  const auto isnan = (x & (uint16_t)0x7fff) > infBits;
  return isnan ? (UV)(uint16_t)0x7fff : x;
}

// Per datatype: the fp32 accumulator of a 16-byte pack, a 4-byte pack and one element, widened exactly and
// rounded back once. bf16 rounds with v_cvt_pk_bf16_f32 (RNE, f32 denormals kept) as nexr_types.hpp does.
template <int D> struct Sym;

template <> struct Sym<nexrFloat32> {
  static constexpr int kEsz = 4;
  using A16 = f32x4;
  using A4 = float;
  using E = uint32_t;
  __device__ static A16 widen16(u32x4 x) { return bc<f32x4>(x); }
  __device__ static u32x4 narrow16(A16 a) { return bc<u32x4>(a); }
  __device__ static A4 widen4(uint32_t x) { return bc<float>(x); }
  __device__ static uint32_t narrow4(A4 a) { return bc<uint32_t>(a); }
  __device__ static float widen1(E x) { return bc<float>(x); }
  __device__ static E narrow1(float a) { return bc<uint32_t>(a); }
};

template <> struct Sym<nexrFloat16> {
  static constexpr int kEsz = 2;
  using A16 = f32x8;
  using A4 = f32x2;
  using E = uint16_t;
  __device__ static A16 widen16(u32x4 x) { return __builtin_convertvector(bc<f16x8>(x), f32x8); }
  __device__ static u32x4 narrow16(A16 a) {
    return bc<u32x4>(sym_canon(bc<u16x8>(__builtin_convertvector(a, f16x8)), 0x7c00));
  }
  __device__ static A4 widen4(uint32_t x) { return __builtin_convertvector(bc<f16x2>(x), f32x2); }
  __device__ static uint32_t narrow4(A4 a) {
    return bc<uint32_t>(sym_canon(bc<u16x2>(__builtin_convertvector(a, f16x2)), 0x7c00));
  }
  __device__ static float widen1(E x) { return (float)bc<_Float16>(x); }
  __device__ static E narrow1(float a) {
    const uint16_t h = bc<uint16_t>((_Float16)a);
    return (h & 0x7fff) > 0x7c00 ? (uint16_t)0x7fff : h;
  }
};

template <> struct Sym<nexrBfloat16> {
  static constexpr int kEsz = 2;
  using A16 = f32x8;
  using A4 = f32x2;
  using E = uint16_t;
  __device__ static A16 widen16(u32x4 x) { return Ty<nexrBfloat16>::widen(bc<u16x8>(x)); }
  __device__ static u32x4 narrow16(A16 a) {
    return bc<u32x4>(sym_canon(bc<u16x8>(__builtin_convertvector(a, bf16x8)), 0x7f80));
  }
  __device__ static A4 widen4(uint32_t x) { return bc<f32x2>((u32x2){x << 16, x & 0xffff0000u}); }
  __device__ static uint32_t narrow4(A4 a) {
    return bc<uint32_t>(sym_canon(bc<u16x2>(__builtin_convertvector(a, bf16x2)), 0x7f80));
  }
  __device__ static float widen1(E x) { return bc<float>((uint32_t)x << 16); }
  __device__ static E narrow1(float a) {
    const f32x2 two = {a, 0.0f};
    const uint16_t h = bc<u16x2>(__builtin_convertvector(two, bf16x2)).x;
    return (h & 0x7fff) > 0x7f80 ? (uint16_t)0x7fff : h;
  }
};

// One piece of a pass: kPacks packs per lane, kStride bytes apart, for the wave that owns it. Pack is the
// access type (the unaligned-capable 16-byte or 4-byte form), Acc its fp32 accumulator.
template <typename Acc, typename Bits, typename LoadPtr, typename StorePtr, int kStride, typename Widen,
          typename Narrow>
__device__ __forceinline__ void sym_piece(const SymParams& P, uint32_t own, uint64_t off, Widen widen,
                                          Narrow narrow) {
  const uint32_t n = (uint32_t)P.nRanks, nFold = (uint32_t)P.nFold;
  Acc acc[2];
  uint32_t r = own;
  for (uint32_t base = 0; base < nFold; base += kSymPeers) {  // wave-uniform, as everything below
    Bits v[kSymPeers][2];
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nFold) {
        const char* p = P.in[r] + off;  // scalar load of the pointer
        v[j][0] = *(LoadPtr*)(p);
        v[j][1] = *(LoadPtr*)(p + kStride);
        r = r + 1 == n ? 0 : r + 1;
      }
    }
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nFold) {
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const Acc a = widen(v[j][u]);
          if (j == 0 && base == 0) acc[u] = a;  // the owner's own input
          else acc[u] = acc[u] + a;             // accumulator first
        }
      }
    }
  }
  const Bits out0 = narrow(acc[0]), out1 = narrow(acc[1]);
  r = own;
  for (uint32_t k = 0; k < n; k++) {  // out[o], out[o + 1], ...
    char* q = P.out[r] + off;
    *(StorePtr*)(q) = out0;
    *(StorePtr*)(q + kStride) = out1;
    r = r + 1 == n ? 0 : r + 1;
  }
}

// A group of 32 end elements, one per lane of the wave's low half.
template <int D>
__device__ __forceinline__ void sym_ends(const SymParams& P, uint32_t own, uint64_t e0, uint32_t lane) {
  using S = Sym<D>;
  using E = typename S::E;
  using LoadPtr = typename std::conditional<S::kEsz == 2, g_cu16, g_cu32>::type;
  using StorePtr = typename std::conditional<S::kEsz == 2, g_u16, g_u32>::type;
  const uint64_t e = e0 + lane;
  if (lane >= kSymEndGroup || e >= P.nEnds) return;
  const uint64_t off = e < P.preElts ? e * S::kEsz : P.sufOff + (e - P.preElts) * S::kEsz;
  const uint32_t n = (uint32_t)P.nRanks, nFold = (uint32_t)P.nFold;
  float acc = 0.0f;
  uint32_t r = own;
  for (uint32_t base = 0; base < nFold; base += kSymPeers) {
    E v[kSymPeers];
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nFold) {
        v[j] = *(LoadPtr*)(P.in[r] + off);
        r = r + 1 == n ? 0 : r + 1;
      }
    }
#pragma unroll
    for (int j = 0; j < kSymPeers; j++) {
      if (base + j < nFold) {
        const float a = S::widen1(v[j]);
        if (j == 0 && base == 0) acc = a;
        else acc = acc + a;
      }
    }
  }
  const E out = S::narrow1(acc);
  r = own;
  for (uint32_t k = 0; k < n; k++) {
    *(StorePtr*)(P.out[r] + off) = out;
    r = r + 1 == n ? 0 : r + 1;
  }
}

// i % n for a wave-uniform i: the 32-bit division whenever i fits (always, below 2 TiB per rank)
__device__ __forceinline__ uint32_t sym_owner(uint64_t i, uint32_t n) {
  return (i >> 32) ? (uint32_t)(i % n) : (uint32_t)i % n;
}

template <int D>
__global__ __launch_bounds__(kBlock) void sym_all_reduce_kernel(SymParams P) {
  using S = Sym<D>;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks;
  const uint64_t p1 = P.p1Pieces, p2 = P.p2Pieces;
  const uint64_t nItems = p1 + p2 + (P.nEnds + kSymEndGroup - 1) / kSymEndGroup;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
    if (it < p1) {
      sym_piece<typename S::A16, u32x4, g_cu32x4_a1, g_u32x4_a1, kSymPiece16 / 2>(
          P, sym_owner(it, n), P.p1Off + it * kSymPiece16 + lane * 16u, [](u32x4 x) { return S::widen16(x); },
          [](typename S::A16 a) { return S::narrow16(a); });
    } else if (it < p1 + p2) {
      const uint64_t i = it - p1;
      sym_piece<typename S::A4, uint32_t, g_cu32_a1, g_u32_a1, kSymPiece4 / 2>(
          P, sym_owner(i, n), P.p2Off + i * kSymPiece4 + lane * 4u, [](uint32_t x) { return S::widen4(x); },
          [](typename S::A4 a) { return S::narrow4(a); });
    } else {
      const uint64_t g = it - p1 - p2;
      sym_ends<D>(P, sym_owner(g, n), g * kSymEndGroup, lane);
    }
  }
}

// ---- ReduceScatter_LD and AllGather_ST (nexrSymReduceScatter, nexrSymAllGather) -----------------------------
// ncclSymRun_ReduceScatter_LD (reference src/device/symmetric/reduce_scatter.hh:6-241) and
// ncclSymRun_AllGather_ST (symmetric/all_gather.hh:5-177) on the same terms as the all-reduce above: ranks on
// this GPU, the barriers at both ends (:234-240, :170-176) the stream's order. Rank r's chunk is a run of
// chunkBytes bytes; nothing about it is shared between ranks, so the reference's pass ladder and CTA count
// (reduce_scatter.hh:160-220) only spread a rank's elements over its own warps, and the layout here is free:
// every chunk is cut from its byte 0, with no head, into
//   pieces   whole 2048-byte pieces, two 16-byte packs per lane 1024 bytes apart (as sym_piece);
//   packs    the remainder below 2048 bytes as 16-byte packs, one per lane, in groups of 64;
//   tail     the last bytes below 16, one element (ReduceScatter) or one byte (AllGather) per lane.
// An item is (rank, piece | group | tail), numbered with the rank fastest (item i is rank i mod n's item
// i / n) so that a grid of few waves still touches every rank; a wave takes whole items, so the rank is
// wave-uniform and the pointers are scalar loads. A chunk's phase is (inputs[s] + r * chunkBytes) mod 16,
// which differs by rank and by count: every pack access is the unaligned-capable form. Offsets are 64-bit
// (r * chunkBytes passes 4 GiB). No LDS, no cross-lane traffic, plain cache policy.

// item i -> (i / n, i mod n) for a wave-uniform i: the 32-bit division whenever i fits
__device__ __forceinline__ void sym_split(uint64_t i, uint32_t n, uint64_t* k, uint32_t* r) {
  if (i >> 32) {
    *k = i / n;
    *r = (uint32_t)(i % n);
  } else {
    *k = (uint32_t)i / n;
    *r = (uint32_t)i % n;
  }
}

// K peers' packs of one wave, straight-line: the K * kPacks loads (kPacks packs per lane, kStride bytes apart,
// at byte `off` of the inputs of ranks r, r + 1, ...), then the adds, the accumulator first. kFirst: the first
// of them is the chunk's own rank and starts the accumulator. Bits is the pack as loaded, LoadPtr its access
// type, Acc its fp32 accumulator.
template <int K, bool kFirst, typename Acc, typename Bits, typename LoadPtr, int kPacks, int kStride, typename Widen>
__device__ __forceinline__ void sym_fold_k(const SymRsParams& P, uint32_t& r, uint64_t off, Widen widen,
                                           Acc (&acc)[kPacks]) {
  const uint32_t n = (uint32_t)P.nRanks;
  Bits v[K][kPacks];
#pragma unroll
  for (int j = 0; j < K; j++) {
    const char* p = P.in[r] + off;  // scalar load of the pointer
#pragma unroll
    for (int u = 0; u < kPacks; u++) v[j][u] = *(LoadPtr*)(p + u * kStride);
    r = r + 1 == n ? 0 : r + 1;
  }
#pragma unroll
  for (int j = 0; j < K; j++) {
#pragma unroll
    for (int u = 0; u < kPacks; u++) {
      const Acc a = widen(v[j][u]);
      if (kFirst && j == 0) acc[u] = a;
      else acc[u] = acc[u] + a;
    }
  }
}

// The fold of a chunk's packs from rank `first` on: a wave-uniform switch on the number of peers, so that
// every case is the loads of up to kSymPeers peers and then the adds with no branch between them; beyond
// kSymPeers ranks the fold goes on in groups of kSymPeers, the last part in groups of 4, 2 and 1.
template <typename Acc, typename Bits, typename LoadPtr, int kPacks, int kStride, typename Widen>
__device__ __forceinline__ void sym_fold(const SymRsParams& P, uint32_t first, uint64_t off, Widen widen,
                                         Acc (&acc)[kPacks]) {
  static_assert(kSymPeers == 8, "the switch below");
  uint32_t r = first, left = (uint32_t)P.nFold;
#define NEXR_SYM_CASE(K)                                                                 \
  case K:                                                                                \
    sym_fold_k<K, true, Acc, Bits, LoadPtr, kPacks, kStride>(P, r, off, widen, acc);     \
    left -= K;                                                                           \
    break;
  switch (left < kSymPeers ? left : (uint32_t)kSymPeers) {
    NEXR_SYM_CASE(1) NEXR_SYM_CASE(2) NEXR_SYM_CASE(3) NEXR_SYM_CASE(4)
    NEXR_SYM_CASE(5) NEXR_SYM_CASE(6) NEXR_SYM_CASE(7) NEXR_SYM_CASE(8)
  }
#undef NEXR_SYM_CASE
  for (; left >= kSymPeers; left -= kSymPeers)
    sym_fold_k<kSymPeers, false, Acc, Bits, LoadPtr, kPacks, kStride>(P, r, off, widen, acc);
  if (left & 4) sym_fold_k<4, false, Acc, Bits, LoadPtr, kPacks, kStride>(P, r, off, widen, acc);
  if (left & 2) sym_fold_k<2, false, Acc, Bits, LoadPtr, kPacks, kStride>(P, r, off, widen, acc);
  if (left & 1) sym_fold_k<1, false, Acc, Bits, LoadPtr, kPacks, kStride>(P, r, off, widen, acc);
}

// ReduceScatter_LD: outputs[r][e] = in[r][r * nElts + e] + in[r + 1][...] + ..., the accumulator first, in
// fp32, rounded once (reduceDeep :23-89, reduceEnds :118-157; the chunk of rank r at :237). A lane loads its
// bytes from every input before it stores them, so outputs[r] may be chunk r of any rank's input.
template <int D>
__global__ __launch_bounds__(kBlock) void sym_reduce_scatter_kernel(SymRsParams P) {
  using S = Sym<D>;
  using E = typename S::E;
  using A16 = typename S::A16;
  using ELoad = typename std::conditional<S::kEsz == 2, g_cu16, g_cu32>::type;
  using EStore = typename std::conditional<S::kEsz == 2, g_u16, g_u32>::type;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks;
  const uint64_t chunk = P.chunkBytes;
  const uint64_t pieces = chunk / kSymPiece16;
  const uint32_t rem = (uint32_t)(chunk % kSymPiece16), packs = rem / 16u, tail = (rem % 16u) / S::kEsz;
  const uint32_t groups = (packs + 63u) / 64u;
  const uint64_t nItems = (pieces + groups + (tail ? 1u : 0u)) * n;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  const auto widen16 = [](u32x4 x) { return S::widen16(x); };
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
    uint64_t k;
    uint32_t r;
    sym_split(it, n, &k, &r);
    const uint64_t at = (uint64_t)r * chunk;  // chunk r of every input
    if (k < pieces) {
      const uint64_t o = k * kSymPiece16 + lane * 16u;
      A16 acc[2];
      sym_fold<A16, u32x4, g_cu32x4_a1, 2, kSymPiece16 / 2>(P, r, at + o, widen16, acc);
      char* q = P.out[r] + o;
      *(g_u32x4_a1*)(q) = S::narrow16(acc[0]);
      *(g_u32x4_a1*)(q + kSymPiece16 / 2) = S::narrow16(acc[1]);
    } else if (k < pieces + groups) {
      const uint32_t p = (uint32_t)(k - pieces) * 64u + lane;
      if (p < packs) {
        const uint64_t o = pieces * kSymPiece16 + p * 16u;
        A16 acc[1];
        sym_fold<A16, u32x4, g_cu32x4_a1, 1, 0>(P, r, at + o, widen16, acc);
        *(g_u32x4_a1*)(P.out[r] + o) = S::narrow16(acc[0]);
      }
    } else if (lane < tail) {
      const uint64_t o = pieces * kSymPiece16 + packs * 16u + lane * S::kEsz;
      float acc[1];
      sym_fold<float, E, ELoad, 1, 0>(P, r, at + o, [](E x) { return S::widen1(x); }, acc);
      *(EStore*)(P.out[r] + o) = S::narrow1(acc[0]);
    }
  }
}

// AllGather_ST: outputs[s][r * nBytes + b] = inputs[r][b], a bit copy (the reference runs it on char, :173).
// One load of the item, then a store to every rank from r on; rank r's own output is skipped when its input
// already lies there (the reference's inPlace, :105, :33, :81: bit r of P.inPlace).
__global__ __launch_bounds__(kBlock) void sym_all_gather_kernel(SymAgParams P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks;
  const uint64_t chunk = P.nBytes;
  const uint64_t pieces = chunk / kSymPiece16;
  const uint32_t rem = (uint32_t)(chunk % kSymPiece16), packs = rem / 16u, tail = rem % 16u;
  const uint32_t groups = (packs + 63u) / 64u;
  const uint64_t nItems = (pieces + groups + (tail ? 1u : 0u)) * n;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
    uint64_t k;
    uint32_t r;
    sym_split(it, n, &k, &r);
    const uint64_t at = (uint64_t)r * chunk;  // chunk r of every output
    const uint32_t skip = (uint32_t)(P.inPlace >> r) & 1u;
    uint32_t s = skip ? (r + 1 == n ? 0 : r + 1) : r;  // out[r], out[r + 1], ...
    if (k < pieces) {
      const uint64_t o = k * kSymPiece16 + lane * 16u;
      const char* p = P.in[r] + o;
      const u32x4 v0 = *(g_cu32x4_a1*)(p), v1 = *(g_cu32x4_a1*)(p + kSymPiece16 / 2);
#pragma unroll 4
      for (uint32_t j = skip; j < n; j++) {
        char* q = P.out[s] + at + o;
        *(g_u32x4_a1*)(q) = v0;
        *(g_u32x4_a1*)(q + kSymPiece16 / 2) = v1;
        s = s + 1 == n ? 0 : s + 1;
      }
    } else if (k < pieces + groups) {
      const uint32_t i = (uint32_t)(k - pieces) * 64u + lane;
      if (i < packs) {
        const uint64_t o = pieces * kSymPiece16 + i * 16u;
        const u32x4 v = *(g_cu32x4_a1*)(P.in[r] + o);
        for (uint32_t j = skip; j < n; j++) {
          *(g_u32x4_a1*)(P.out[s] + at + o) = v;
          s = s + 1 == n ? 0 : s + 1;
        }
      }
    } else if (lane < tail) {
      const uint64_t o = pieces * kSymPiece16 + packs * 16u + lane;
      const uint8_t v = *(g_cu8*)(P.in[r] + o);
      for (uint32_t j = skip; j < n; j++) {
        *(g_u8*)(P.out[s] + at + o) = v;
        s = s + 1 == n ? 0 : s + 1;
      }
    }
  }
}

// ---- the LL members: AllReduce_AGxLL_R, ReduceScatter_LL, AllGather_LL (nexrSymLL*) -------------------------
// ncclSymRun_AllReduce_AGxLL_R (reference src/device/symmetric/all_reduce.hh:356-428), ncclSymRun_ReduceScatter_LL
// (reduce_scatter.hh:320-388) and ncclSymRun_AllGather_LL (all_gather.hh:256-363) over sendLL / bcastLL /
// recvLL / recvReduceLL / endLL (symmetric/primitives.hh:212-377), for ranks on this GPU. The rules and the
// window layout are in include/nexr.h; what is kept of the protocol is the per-block epoch word that outlives
// the call, the two line buffers chosen by the flag's parity, the broadcast of a rank's packs into every
// window, the rank-0-first fp32 fold and the cleanup at the wrap. Inside the line area the layout is free.
//
// A team is one workgroup, (rank w mod n, block w / n) of a grid of n * B. It takes its share of the 8-byte
// packs (the reference's split: P / B, one more for b < P mod B) in rounds of kSymLLRound = kBlock packs,
// ONE pack per lane and round: the lane loads its pack with a plain load, stores it as the line
// {lo, f, hi, f} into slot rank * kSymLLRound + lane of the parity-f buffer of block b in every window (the
// reduce-scatter: pack p of chunk s into window s), then polls slots j * kSymLLRound + lane, j = 0..n-1, of
// its OWN window, kSymPeers lines in flight, folds them in rank order and stores the result with a plain
// store. A line is one 16-byte sc0 sc1 buffer store and one such load per try (wire_st / wire_ld). The round
// ends with a workgroup barrier: no lane of a rank sends round k + 1 before all of that rank's team have read
// round k, and a peer's round k + 2 lines (the same buffer) follow its receipt of this team's round k + 1
// lines. A poll is bounded as wait_head is; a lane whose poll gave up marks the team dead in LDS, and from
// the next barrier on the team skips its polls and stores but still sends and still reaches every barrier.
constexpr int kSymLLRound = NEXR_SYM_LL_ROUND_PACKS;
static_assert(kSymLLRound == kBlock, "one pack per lane and round");
enum { kSymLLAllReduce = 0, kSymLLReduceScatter = 1, kSymLLAllGather = 2 };

__device__ __forceinline__ bool sym_ll_match(u32x4 x, uint32_t f) { return x.y == f && x.w == f; }

// recvLL's loop (primitives.hh:302-335) for one line that was not there at the first try
__device__ __forceinline__ bool sym_ll_poll(__amdgpu_buffer_rsrc_t r, uint32_t off, uint32_t f, u32x4& x,
                                            uint64_t timeoutTicks, uint32_t* status) {
  uint64_t t0 = 0;
  for (uint32_t tries = 1;; tries++) {
    __builtin_amdgcn_s_sleep(1);
    x = wire_ld(r, off);
    if (sym_ll_match(x, f)) return true;
    if (tries % kLLAbortEvery == 0 && ll_aborted(status)) return false;
    if (tries % kLLClockEvery) continue;
    const uint64_t now = __builtin_amdgcn_s_memrealtime();
    if (!t0) t0 = now;
    else if (now - t0 > timeoutTicks) {
      if (status) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
  }
}

template <int K, int D>
__device__ __forceinline__ void sym_ll_team(const SymLLParams& P) {
  using S = Sym<D>;
  using A4 = typename S::A4;
  __shared__ uint32_t teamDead;
  const uint32_t n = (uint32_t)P.nRanks, B = (uint32_t)P.nBlocks;
  const uint32_t rank = blockIdx.x % n, blk = blockIdx.x / n;  // rank fastest
  const uint32_t t = threadIdx.x;
  const uint64_t nBytes = P.nBytes;
  const uint32_t packs = (uint32_t)((nBytes + 7) / 8);  // the host keeps nBytes below 2^31
  const uint32_t share = packs / B + (blk < packs % B ? 1u : 0u);
  const uint32_t first = blk * (packs / B) + (blk < packs % B ? blk : packs % B);
  if (share == 0) return;  // the whole team: no round, the epoch word stays
  if (t == 0) teamDead = 0;
  char* mine = P.win[rank];
  g_u32* word = (g_u32*)mine + blk;
  uint32_t f = __builtin_amdgcn_readfirstlane(*word) + 2u;
  const uint32_t bufBytes = n * kSymLLRound * 16u;
  bool dead = false, bad = false;
  __syncthreads();
  for (uint32_t done = 0; done < share; done += kSymLLRound) {
    const bool have = t < share - done;
    const uint32_t p = first + done + t;
    const uint64_t lines = NEXR_SYM_LL_HEADER_BYTES + (uint64_t)(blk * 2u + (f & 1u)) * bufBytes;
    // bcastLL / sendLL: own window first, then rank + 1, ...
    if (have) {
      uint64_t d = 0;
      if (K != kSymLLReduceScatter) d = ld_line(P.in[rank], p, nBytes);
      uint32_t s = rank;
      for (uint32_t k = 0; k < n; k++) {
        if (K == kSymLLReduceScatter) d = ld_line(P.in[rank] + (uint64_t)s * nBytes, p, nBytes);
        wire_st(wire_rsrc(P.win[s] + lines, bufBytes), (rank * kSymLLRound + t) * 16u,
                (u32x4){(uint32_t)d, f, (uint32_t)(d >> 32), f});
        s = s + 1 == n ? 0 : s + 1;
      }
    }
    const auto own = wire_rsrc(mine + lines, bufBytes);
    if (have && !dead) {
      A4 lo, hi;
      for (uint32_t base = 0; base < n; base += kSymPeers) {  // team-uniform
        u32x4 v[kSymPeers];
#pragma unroll
        for (int j = 0; j < kSymPeers; j++)  // all in flight, no branch between them; past rank n - 1 the
          v[j] = wire_ld(own, ((base + j) * kSymLLRound + t) * 16u);  // descriptor clips: zeros, no access
#pragma unroll
        for (int j = 0; j < kSymPeers; j++) {
          if (base + j < n && !bad) {
            if (!sym_ll_match(v[j], f))
              bad = !sym_ll_poll(own, ((base + j) * kSymLLRound + t) * 16u, f, v[j], P.timeoutTicks, P.status);
            if (bad) continue;
            if (K == kSymLLAllGather) {
              st_line(P.out[rank] + (uint64_t)(base + j) * nBytes, p, nBytes, (uint64_t)v[j].z << 32 | v[j].x);
            } else {  // recvReduceLL: rank 0 first, the accumulator first
              const A4 a = S::widen4(v[j].x), b = S::widen4(v[j].z);
              if (j == 0 && base == 0) lo = a, hi = b;
              else if (!P.firstWins) lo = lo + a, hi = hi + b;
            }
          }
        }
      }
      if (K != kSymLLAllGather && !bad)
        st_line(P.out[rank], p, nBytes, (uint64_t)S::narrow4(hi) << 32 | S::narrow4(lo));
    }
    if (bad) teamDead = 1;
    // endLL: at the wrap this parity's buffer is zeroed, after everybody's reads and drained before the barrier
    if (f >= 0xfffffffeu) {
      __syncthreads();
      for (uint32_t i = t; i < n * kSymLLRound; i += kBlock) wire_st(own, i * 16u, (u32x4){0u, 0u, 0u, 0u});
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    dead = teamDead != 0;
    f = f == 0xffffffffu ? 2u : f + 1u;
  }
  if (t == 0) *word = f - 2u;
}

template <int D>
__global__ __launch_bounds__(kBlock) void sym_ll_all_reduce_kernel(SymLLParams P) {
  sym_ll_team<kSymLLAllReduce, D>(P);
}
template <int D>
__global__ __launch_bounds__(kBlock) void sym_ll_reduce_scatter_kernel(SymLLParams P) {
  sym_ll_team<kSymLLReduceScatter, D>(P);
}
__global__ __launch_bounds__(kBlock) void sym_ll_all_gather_kernel(SymLLParams P) {
  sym_ll_team<kSymLLAllGather, nexrFloat32>(P);  // a bit copy: the datatype is not used
}

static const void* sym_ll_fn(int coll, int dt) {
  if (coll == kSymLLAllGather) return (const void*)&sym_ll_all_gather_kernel;
  if (coll == kSymLLAllReduce)
    return dt == nexrFloat32    ? (const void*)&sym_ll_all_reduce_kernel<nexrFloat32>
           : dt == nexrFloat16  ? (const void*)&sym_ll_all_reduce_kernel<nexrFloat16>
           : dt == nexrBfloat16 ? (const void*)&sym_ll_all_reduce_kernel<nexrBfloat16>
                                : nullptr;
  if (coll == kSymLLReduceScatter)
    return dt == nexrFloat32    ? (const void*)&sym_ll_reduce_scatter_kernel<nexrFloat32>
           : dt == nexrFloat16  ? (const void*)&sym_ll_reduce_scatter_kernel<nexrFloat16>
           : dt == nexrBfloat16 ? (const void*)&sym_ll_reduce_scatter_kernel<nexrBfloat16>
                                : nullptr;
  return nullptr;
}

hipError_t launch_sym_ll(int coll, int dt, const SymLLParams& p, hipStream_t s) {
  const void* fn = sym_ll_fn(coll, dt);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<SymLLParams*>(&p)};
  return hipLaunchKernel(fn, dim3((unsigned)(p.nRanks * p.nBlocks)), dim3(kBlock), args, 0, s);
}

hipError_t sym_ll_blocks_per_cu(int coll, int dt, int* blocks) {
  const void* fn = sym_ll_fn(coll, dt);
  if (!fn) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, kBlock, 0);
}

hipError_t launch_sym_reduce_scatter(int dt, const SymRsParams& p, unsigned grid, hipStream_t s) {
  const void* fn = dt == nexrFloat32    ? (const void*)&sym_reduce_scatter_kernel<nexrFloat32>
                   : dt == nexrFloat16  ? (const void*)&sym_reduce_scatter_kernel<nexrFloat16>
                   : dt == nexrBfloat16 ? (const void*)&sym_reduce_scatter_kernel<nexrBfloat16>
                                        : nullptr;
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<SymRsParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_sym_all_gather(const SymAgParams& p, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<SymAgParams*>(&p)};
  return hipLaunchKernel((const void*)&sym_all_gather_kernel, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_sym_all_reduce(int dt, const SymParams& p, unsigned grid, hipStream_t s) {
  const void* fn = dt == nexrFloat32    ? (const void*)&sym_all_reduce_kernel<nexrFloat32>
                   : dt == nexrFloat16  ? (const void*)&sym_all_reduce_kernel<nexrFloat16>
                   : dt == nexrBfloat16 ? (const void*)&sym_all_reduce_kernel<nexrBfloat16>
                                        : nullptr;
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<SymParams*>(&p)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

}  // namespace nexr
