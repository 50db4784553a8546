// nexr_ll.hip — the LL-protocol reduce-copy for gfx950.
//
// What it computes is LLGenericOp<RECV, SEND, SrcBuf, DstBuf> (reference src/device/prims_ll.h:
// 218-283) for one FIFO step whose slot pointers and flags the caller resolved:
//   per 8-byte data line l:  d = src[l] (applyPreOp with redOpArg when the source is the user input)
//                            d = RECV ? (SRC ? op(peer0[l], d) : peer0[l]) : d
//                            d = op(peer_i[l], d) for i = 1..nRecv-1      (peer is the FIRST operand)
//                            d = postOp ? applyPostOp(d) : d
//                            send_i[l] = {lo32(d), flag_i, hi32(d), flag_i}   (storeLL :152-158)
//                            dst[l] = d (only the line's valid elements, storeData :202-216)
// A recv line is valid when both its flags equal the expected step flag (readLL :91-109); the
// kernel polls them with system-scope relaxed 64-bit loads, bounded in time, and reports a
// timeout through the optional status word instead of hanging (checkAbort, primitives.h:142-156).
//
// A run of such steps in one launch, with waitSend / postRecv on device head words (nexrReduceCopyLLSteps,
// reduce_copy_ll_steps_kernel below), and the LL128 step at the end of the file.
//
// MI355X mapping: one lane handles two lines 64 apart (one 16-byte data pack, so the LL path reuses
// the SIMPLE path's per-datatype pack arithmetic, nexr_types.hpp, unchanged) and moves each line as
// one 16-byte system-coherent access; a wave instruction covers 1 KiB of contiguous wire. Lines
// whose flags are not there yet fall back to the polling loop.
#include "nexr_types.hpp"

namespace nexr {

typedef __attribute__((address_space(1))) uint64_t g_u64;
typedef uint64_t __attribute__((aligned(1))) u64_a1;  // user-buffer words at any alignment (nexr_types.hpp)
typedef __attribute__((address_space(1))) u64_a1 g_u64_a1;

__device__ __forceinline__ uint64_t ld_sys(const char* p) {
  return __hip_atomic_load((const g_u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys(char* p, uint64_t v) {
  __hip_atomic_store((g_u64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Wire accesses on the fast path: one 16-byte buffer load / store per LL line or LL128 wire unit,
// with the same system-coherence bits (sc0 sc1) as the 8-byte atomics above, through a descriptor
// built per tile from a wave-uniform base (the descriptor's size also clips the last tile). A 16-B
// access moves both 8-byte {data, flag} granules of a line in one instruction; each granule is
// written and read whole (MI355X_MICROARCH.md, hand-offs: "R2's granule ... untorn ... also for
// 16-B sc1 halves"), which is the LL protocol's own requirement (prims_ll.h:91-109, :152-158).
#ifndef NEXR_LL_LOAD_BITS  // overridable only by tuning harnesses (tools/ll_bits.hip)
#define NEXR_LL_LOAD_BITS 17
#endif
#ifndef NEXR_LL_STORE_BITS
#define NEXR_LL_STORE_BITS 17
#endif
constexpr int kLoadBits = NEXR_LL_LOAD_BITS;    // raw_buffer aux bits: bit 0 sc0, bit 4 sc1
constexpr int kStoreBits = NEXR_LL_STORE_BITS;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wire_rsrc(const char* base, uint64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 wire_ld(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return bc<u32x4>(__builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kLoadBits));
}
__device__ __forceinline__ void wire_st(__amdgpu_buffer_rsrc_t r, uint32_t off, u32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kStoreBits);
}

#ifndef NEXR_LL_CLOCK_EVERY  // overridable only by tuning harnesses (tools/ll_steps_trace.hip)
#define NEXR_LL_CLOCK_EVERY 1
#endif
constexpr uint32_t kLLClockEvery = NEXR_LL_CLOCK_EVERY;
// A poll that keeps failing also reads the status word now and then (every kLLAbortEvery tries, a read
// over PCIe when the word is pinned host memory): non-zero means another step timed out or the caller
// aborted (checkAbort, primitives.h:142-156), and the poll gives up at once instead of at its timeout.
constexpr uint32_t kLLAbortEvery = 64;
__device__ __forceinline__ bool ll_aborted(const uint32_t* status) {
  return status && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}
#ifndef NEXR_LL_POLL_PIPE  // the same: two tries of a line poll in flight (1) or one (0)
#define NEXR_LL_POLL_PIPE 0
#endif
#ifndef NEXR_LL_POLL_SLEEP  // the same: s_sleep between two tries of a line poll
#define NEXR_LL_POLL_SLEEP 1
#endif

// The first n (<= 16) bytes at p as a zero-padded pack, and the reverse: byte accesses assembled in
// registers (a variable-length memcpy into a register array would put the array on the stack).
__device__ __forceinline__ u32x4 ld_partial(const char* p, uint64_t n) {
  if (n == 8) {  // an LL128 flag lane's half chunk
    const uint64_t x = *(const g_u64_a1*)p;
    return (u32x4){(uint32_t)x, (uint32_t)(x >> 32), 0u, 0u};
  }
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; k++)
    if ((uint64_t)k < n) w[k >> 2] |= (uint32_t)(uint8_t)p[k] << (8 * (k & 3));
  return (u32x4){w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ void st_partial(char* p, uint64_t n, u32x4 v) {
  if (n == 8) {
    *(g_u64_a1*)p = (uint64_t)v.y << 32 | v.x;
    return;
  }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 16; k++)
    if ((uint64_t)k < n) p[k] = (char)(w[k >> 2] >> (8 * (k & 3)));
}

// 8 data bytes of line l of a user buffer (fewer at its end; any alignment: unaligned 8-B
// accesses, as the SIMPLE path's unaligned 16-B ones), and the reverse.
__device__ __forceinline__ uint64_t ld_line(const char* p, uint64_t l, uint64_t nBytes) {
  const char* q = p + l * 8;
  const uint64_t v = nBytes - l * 8;
  if (v >= 8) return *(const g_u64_a1*)q;
  const u32x4 x = ld_partial(q, v);
  return (uint64_t)x.y << 32 | x.x;
}
__device__ __forceinline__ void st_line(char* p, uint64_t l, uint64_t nBytes, uint64_t x) {
  char* q = p + l * 8;
  const uint64_t v = nBytes - l * 8;
  if (v >= 8) *(g_u64_a1*)q = x;
  else st_partial(q, v, (u32x4){(uint32_t)x, (uint32_t)(x >> 32), 0u, 0u});
}

// One tile = kLLU sub-tiles of 2 * kBlock lines. In a sub-tile, wave w owns lines [128w, 128w + 128)
// and lane j of it lines 128w + j and 128w + j + 64, so every wave instruction touches 1 KiB of
// contiguous wire (or 512 B of user buffer). The lane's two lines form one 16-byte pack {line0,
// line1}: the reduction is element-wise, so the SIMPLE path's pack arithmetic (nexr_types.hpp)
// applies unchanged. All kLLU sub-tiles' loads of one buffer are issued before any is used.

// Returns false when one of this lane's lines never arrived (status set; its outputs unwritten).
// A: LLParams (one step, read from the kernel arguments) or LLStepArgs (a step of a run, built in
// registers: its peer loops are unrolled over MaxPeers so that no array is indexed at run time).
template <int D, int OP, bool IsMin, typename A = LLParams, int MaxPeers = 1>
__device__ __forceinline__ bool ll_tile(const A& a, uint64_t tile, uint64_t nBytes, uint64_t nLines) {
  using T = Ty<D>;
  using V = typename T::V;
  const uint64_t L0 = tile * kLLTileLines;
  const uint32_t tileLines = (uint32_t)(nLines - L0 < (uint64_t)kLLTileLines ? nLines - L0 : kLLTileLines);
  const uint32_t o0 = (threadIdx.x >> 6) * 128 + (threadIdx.x & 63);
  u32x4 d[kLLU];
  bool ok[kLLU], two[kLLU];
  bool arrived = true;
  // The first peer's lines are loaded before the user's: they wait for the peer (system-coherent, not
  // cached), the user's only for memory, so the two latencies overlap. In a tile whose lines are all
  // whole (every tile but a step's last) the user loads carry no per-line branch, so they go out
  // together too instead of one after another.
  u32x4 p0[kLLU], p1[kLLU];
  if (a.nRecv > 0) {
    const auto r = wire_rsrc(a.recv[0] + L0 * 16, (uint64_t)tileLines * 16);
#pragma unroll
    for (int u = 0; u < kLLU; u++) {  // past the end: zeros
      p0[u] = wire_ld(r, (u * kLLSubLines + o0) * 16);
      p1[u] = wire_ld(r, (u * kLLSubLines + o0 + 64) * 16);
    }
  }
  const bool wholeTile = (L0 + tileLines) * 8 <= nBytes;
#pragma unroll
  for (int u = 0; u < kLLU; u++) {
    const uint32_t m0 = u * kLLSubLines + o0;
    ok[u] = m0 < tileLines;
    two[u] = m0 + 64 < tileLines;
    uint64_t s0 = 0, s1 = 0;
    if (a.src && wholeTile) {
      if (ok[u]) s0 = *(const g_u64_a1*)(a.src + (L0 + m0) * 8);
      if (two[u]) s1 = *(const g_u64_a1*)(a.src + (L0 + m0 + 64) * 8);
    } else if (a.src) {
      if (ok[u]) s0 = ld_line(a.src, L0 + m0, nBytes);
      if (two[u]) s1 = ld_line(a.src, L0 + m0 + 64, nBytes);
    }
    d[u] = (u32x4){(uint32_t)s0, (uint32_t)(s0 >> 32), (uint32_t)s1, (uint32_t)(s1 >> 32)};
    if constexpr (OP == nexrDevPreMulSum) {
      if (a.src && a.srcIsInput) d[u] = bc<u32x4>(T::mul(bc<V>(d[u]), T::splat(a.redArg)));  // applyPreOp
    }
  }
#pragma unroll MaxPeers
  for (int i = 0; i < (MaxPeers > 1 ? MaxPeers : NEXR_MAX_SRCS); i++) {
    if (i >= a.nRecv) break;
    const auto r = wire_rsrc(a.recv[i] + L0 * 16, (uint64_t)tileLines * 16);
    u32x4 x0[kLLU], x1[kLLU];
#pragma unroll
    for (int u = 0; u < kLLU; u++) {  // past the end: zeros
      x0[u] = i == 0 ? p0[u] : wire_ld(r, (u * kLLSubLines + o0) * 16);
      x1[u] = i == 0 ? p1[u] : wire_ld(r, (u * kLLSubLines + o0 + 64) * 16);
    }
    const uint32_t f = a.recvFlag[i];
#pragma unroll
    for (int u = 0; u < kLLU; u++) {
      if (!ok[u]) continue;
      u32x4 peer;
      if (x0[u].y == f && x0[u].w == f && (!two[u] || (x1[u].y == f && x1[u].w == f))) {
        peer = (u32x4){x0[u].x, x0[u].z, x1[u].x, x1[u].z};
      } else {  // not there yet: reload the lane's two lines until both carry the flag (readLL's loop,
                // prims_ll.h:91-109), one 16-B access per line per try, bounded in time
        uint64_t t0 = 0;
        bool got = true;
#if NEXR_LL_POLL_PIPE
        // Two tries in flight: the next one is issued before the current one is looked at, so a line that
        // lands while a try is on its way is seen one sleep later rather than one round trip later.
        u32x4 n0 = wire_ld(r, (u * kLLSubLines + o0) * 16), n1 = wire_ld(r, (u * kLLSubLines + o0 + 64) * 16);
#endif
        for (uint32_t tries = 1;; tries++) {
          if (NEXR_LL_POLL_SLEEP) __builtin_amdgcn_s_sleep(NEXR_LL_POLL_SLEEP);
#if NEXR_LL_POLL_PIPE
          x0[u] = n0, x1[u] = n1;
          n0 = wire_ld(r, (u * kLLSubLines + o0) * 16);
          n1 = wire_ld(r, (u * kLLSubLines + o0 + 64) * 16);
#else
          x0[u] = wire_ld(r, (u * kLLSubLines + o0) * 16);
          x1[u] = wire_ld(r, (u * kLLSubLines + o0 + 64) * 16);
#endif
          if (x0[u].y == f && x0[u].w == f && (!two[u] || (x1[u].y == f && x1[u].w == f))) break;
          if (tries % kLLAbortEvery == 0 && ll_aborted(a.status)) {  // checkAbort (primitives.h:142-156)
            got = false;
            break;
          }
          if (tries % kLLClockEvery) continue;  // the clock is a scalar memory read: not on every try
          const uint64_t now = __builtin_amdgcn_s_memrealtime();
          if (!t0) t0 = now;
          else if (now - t0 > a.timeoutTicks) {
            if (a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            got = false;
            break;
          }
        }
        if (!got) {
          ok[u] = false;  // never arrived: status set, this pack's outputs stay unwritten
          arrived = false;
          continue;
        }
        peer = (u32x4){x0[u].x, x0[u].z, x1[u].x, x1[u].z};
      }
      if ((i == 0 && !a.src) || a.firstWins) d[u] = peer;  // SKIP_COMP: applyReduce returns the peer
      else d[u] = bc<u32x4>(reduce_step<D, OP, IsMin>(bc<V>(peer), bc<V>(d[u])));  // applyReduce(op, peer, d)
    }
  }
#pragma unroll
  for (int u = 0; u < kLLU; u++) {
    if constexpr (OP == nexrDevSumPostDiv) {
      if (a.postOp) d[u] = bc<u32x4>(T::divide(bc<V>(d[u]), a.redArg));
    }
    if constexpr (T::kCanon) {
      // ncclFromFloat canonicalises NaN whenever arithmetic ran on the pack
      const bool arith = !a.firstWins && ((a.nRecv >= 1 && a.src) || a.nRecv >= 2 ||
                                          (OP == nexrDevPreMulSum && a.src && a.srcIsInput));
      if (arith) d[u] = bc<u32x4>(T::canon(bc<V>(d[u])));
    }
  }
#pragma unroll MaxPeers
  for (int i = 0; i < (MaxPeers > 1 ? MaxPeers : NEXR_MAX_DSTS); i++) {
    if (i >= a.nSend) break;
    const auto r = wire_rsrc(a.send[i] + L0 * 16, (uint64_t)tileLines * 16);
    const uint32_t f = a.sendFlag[i];
#pragma unroll
    for (int u = 0; u < kLLU; u++) {  // storeLL (prims_ll.h:152-158)
      if (ok[u]) wire_st(r, (u * kLLSubLines + o0) * 16, (u32x4){d[u].x, f, d[u].y, f});
      if (ok[u] && two[u]) wire_st(r, (u * kLLSubLines + o0 + 64) * 16, (u32x4){d[u].z, f, d[u].w, f});
    }
  }
  if (a.dst) {
#pragma unroll
    for (int u = 0; u < kLLU; u++) {
      const uint64_t l0 = L0 + u * kLLSubLines + o0;
      if (ok[u]) st_line(a.dst, l0, nBytes, (uint64_t)d[u].y << 32 | d[u].x);
      if (ok[u] && two[u]) st_line(a.dst, l0 + 64, nBytes, (uint64_t)d[u].w << 32 | d[u].z);
    }
  }
  return arrived;
}

// The flag-wrap cleanup of one slot (reference incSend, prims_ll.h:85-93): lines [nLines, slotLines) of
// the slot become {0, f, 0, f}, through the same 16-byte store as the data lines. Tiles t0, t0 + stride,
// ... of the slot, and in a tile the lines ll_tile gives this lane (wave v: lines [128v, 128v + 128) of
// every 512), so in a run every clean line is written by the wave whose credit covers it; the tile that
// is part data and part clean is split at nLines, and tiles that are all data are skipped.
__device__ __forceinline__ void ll_clean_tiles(char* slot, uint32_t f, uint64_t nLines, uint64_t slotLines,
                                               uint64_t t0, uint64_t stride) {
  const uint32_t o0 = (threadIdx.x >> 6) * 128 + (threadIdx.x & 63);
  const uint64_t slotTiles = (slotLines + kLLTileLines - 1) / kLLTileLines;
  const u32x4 v = (u32x4){0u, f, 0u, f};
  for (uint64_t t = t0; t < slotTiles; t += stride) {
    const uint64_t L0 = t * kLLTileLines;
    if (L0 + kLLTileLines <= nLines) continue;
    const uint32_t tileLines = (uint32_t)(slotLines - L0 < (uint64_t)kLLTileLines ? slotLines - L0 : kLLTileLines);
    const uint32_t first = nLines > L0 ? (uint32_t)(nLines - L0) : 0u;
    const auto r = wire_rsrc(slot + L0 * 16, (uint64_t)tileLines * 16);
#pragma unroll
    for (int u = 0; u < kLLU; u++) {
      const uint32_t m0 = u * kLLSubLines + o0;
      if (m0 >= first && m0 < tileLines) wire_st(r, m0 * 16, v);
      if (m0 + 64 >= first && m0 + 64 < tileLines) wire_st(r, (m0 + 64) * 16, v);
    }
  }
}

// nexrLLCleanSlot: the cleanup for callers of the single-step kernel below, who resolve the flags and
// own the credits themselves.
__global__ __launch_bounds__(kBlock) void ll_clean_kernel(LLCleanParams a) {
  for (int i = 0; i < NEXR_MAX_DSTS; i++) {
    if (i >= a.nSend) break;
    ll_clean_tiles(a.send[i], a.flag[i], a.firstLine, a.slotLines, blockIdx.x, gridDim.x);
  }
}

hipError_t launch_ll_clean(const LLCleanParams& a, int grid, hipStream_t s) {
  void* args[] = {const_cast<LLCleanParams*>(&a)};
  return hipLaunchKernel((const void*)&ll_clean_kernel, dim3(grid), dim3(kBlock), args, 0, s);
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_ll_kernel(LLParams a) {
  const uint64_t nBytes = a.nElts * (16 / Ty<D>::EPP);
  const uint64_t nLines = (nBytes + 7) / 8;
  const uint64_t nTiles = (nLines + kLLTileLines - 1) / kLLTileLines;
  for (uint64_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
    if constexpr (OP == nexrDevMinMax) {
      if ((a.redArg & 1) == 0) ll_tile<D, OP, true>(a, t, nBytes, nLines);
      else ll_tile<D, OP, false>(a, t, nBytes, nLines);
    } else {
      ll_tile<D, OP, false>(a, t, nBytes, nLines);
    }
  }
}

template <int D>
static hipError_t launch_ll_dt(const LLParams& a, int op, int grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (op) {
    case nexrDevSum: fn = (const void*)&reduce_copy_ll_kernel<D, nexrDevSum>; break;
    case nexrDevProd: fn = (const void*)&reduce_copy_ll_kernel<D, nexrDevProd>; break;
    case nexrDevMinMax: fn = (const void*)&reduce_copy_ll_kernel<D, nexrDevMinMax>; break;
    case nexrDevPreMulSum: fn = (const void*)&reduce_copy_ll_kernel<D, nexrDevPreMulSum>; break;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) fn = (const void*)&reduce_copy_ll_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<LLParams*>(&a)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_ll(int dt, const LLParams& a, int op, int grid, hipStream_t s) {
  switch (dt) {
    case nexrInt8: return launch_ll_dt<nexrInt8>(a, op, grid, s);
    case nexrUint8: return launch_ll_dt<nexrUint8>(a, op, grid, s);
    case nexrInt32: return launch_ll_dt<nexrInt32>(a, op, grid, s);
    case nexrUint32: return launch_ll_dt<nexrUint32>(a, op, grid, s);
    case nexrInt64: return launch_ll_dt<nexrInt64>(a, op, grid, s);
    case nexrUint64: return launch_ll_dt<nexrUint64>(a, op, grid, s);
    case nexrFloat16: return launch_ll_dt<nexrFloat16>(a, op, grid, s);
    case nexrFloat32: return launch_ll_dt<nexrFloat32>(a, op, grid, s);
    case nexrFloat64: return launch_ll_dt<nexrFloat64>(a, op, grid, s);
    case nexrBfloat16: return launch_ll_dt<nexrBfloat16>(a, op, grid, s);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// A run of LL steps in one launch (nexrReduceCopyLLSteps): LLGenericOp per step with the credit
// protocol on the device (waitSend / postRecv, reference src/device/prims_ll.h:55-83). The reference
// runs a step with one thread block and one head counter per connection; here a step's line tiles are
// spread over the grid, and inside a tile each wave owns its own lines (ll_tile: wave v, lines
// [128v, 128v + 128) of every 512), the same lines of every slot on both ends of a connection. So the
// credit is per wave: head word (w, v) of a connection tells the sender's wave v of workgroup w how far
// the receiver's wave v of workgroup w has read, and every wave walks the steps on its own, with no
// barrier: no wave ever waits for another wave of its own launch.
// ---------------------------------------------------------------------------------------------
constexpr int kLLWaves = kBlock / 64;
__device__ __forceinline__ uint64_t* head_word(uint64_t* base, uint32_t w) {
  return base + ((size_t)w * kLLWaves + (threadIdx.x >> 6)) * (kLLHeadStride / 8);
}
// waitSend's head poll (:58-62), by every lane of the wave on the same word (one request), bounded like
// the line polls, into the wave's cache of the head (sendConnHeadCache): a fresh read only when the
// cached value does not cover the step. Relaxed: the receiver published the head after its reads of the
// slot were over (their values were in its outputs), and this wave's stores to the slot come after the
// poll returned.
__device__ __forceinline__ bool wait_head(const uint64_t* p, uint64_t need, uint64_t& cache, uint64_t timeoutTicks,
                                          uint32_t* status) {
  if (cache >= need) return true;
  uint64_t t0 = 0;
  for (uint32_t tries = 1;; tries++) {
    cache = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (cache >= need) return true;
    if (tries % kLLAbortEvery == 0 && ll_aborted(status)) return false;
    if (tries % kLLClockEvery == 0) {
      const uint64_t now = __builtin_amdgcn_s_memrealtime();
      if (!t0) t0 = now;
      else if (now - t0 > timeoutTicks) {
        if (status) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

struct LLStepArgs {  // the fields of LLParams that ll_tile reads, for one step of a run
  const char* src;
  char* dst;
  const char* recv[NEXR_LL_STEPS_MAX_PEERS];
  uint32_t recvFlag[NEXR_LL_STEPS_MAX_PEERS];
  char* send[NEXR_LL_STEPS_MAX_PEERS];
  uint32_t sendFlag[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t redArg;
  uint32_t* status;
  uint64_t timeoutTicks;
  int nRecv, nSend, srcIsInput, postOp, firstWins;
};

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_ll_steps_kernel(LLStepsParams P) {
  constexpr uint64_t esz = 16 / Ty<D>::EPP;
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  const uint32_t w = blockIdx.x, G = gridDim.x;
  const bool lead = (threadIdx.x & 63) == 0;
#ifdef NEXR_LL_STEPS_TRACE  // tuning harness only (tools/ll_steps_trace.hip): per-step phase times
  __shared__ uint64_t tr[kLLStepsMax][5];
#define NEXR_TRACE(k, j) \
  if (threadIdx.x == 0) tr[k][j] = __builtin_amdgcn_s_memrealtime()
#else
#define NEXR_TRACE(k, j)
#endif
  // Step counters, their slot indices (kept by increment: a 64-bit modulo per step is a long scalar
  // division) and the wave's cached heads.
  uint64_t rs[MP], ss[MP], headCache[MP];
  uint32_t rSlot[MP], sSlot[MP];
#pragma unroll
  for (int i = 0; i < MP; i++) {
    rs[i] = P.recvStep[i], ss[i] = P.sendStep[i], headCache[i] = 0;
    rSlot[i] = (uint32_t)(rs[i] % (uint64_t)P.nSlots), sSlot[i] = (uint32_t)(ss[i] % (uint64_t)P.nSlots);
  }
  // Every earlier step of this stream has completed: whatever ran them, the slots before recvStep are read.
  if (lead)
    for (int i = 0; i < P.nRecv; i++)
      __hip_atomic_store(head_word(P.recvHead[i], w), rs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  LLStepArgs a;
  a.redArg = P.redArg;
  a.status = P.status;
  a.timeoutTicks = P.timeoutTicks;
  a.firstWins = P.firstWins;
  for (int k = 0; k < P.nSteps; k++) {
    const nexrLLStep& st = P.step[k];  // scalar loads from the kernel arguments (an LDS copy was slower)
    const uint64_t nBytes = (uint64_t)st.nElts * esz;
    const uint64_t nLines = (nBytes + 7) / 8;
    const uint64_t nTiles = (nLines + kLLTileLines - 1) / kLLTileLines;
    NEXR_TRACE(k, 0);
    if (w < nTiles) {
      if (st.send) {  // waitSend: the receiver's wave has read the step nSlots back
#pragma unroll
        for (int j = 0; j < MP; j++)
          if (j < P.nSend && ss[j] + 1 > (uint64_t)P.nSlots &&
              !wait_head(head_word(const_cast<uint64_t*>(P.sendHead[j]), w), ss[j] + 1 - P.nSlots, headCache[j],
                         P.timeoutTicks, P.status))
            return;  // no credit: status set, this wave stops
      }
      a.src = st.srcBuf == 0 ? P.input + st.srcIx * esz : st.srcBuf == 1 ? P.output + st.srcIx * esz : nullptr;
      a.dst = st.dstBuf == 0 ? const_cast<char*>(P.input) + st.dstIx * esz
              : st.dstBuf == 1 ? P.output + st.dstIx * esz : nullptr;
      a.nRecv = st.recv ? P.nRecv : 0;
      a.nSend = st.send ? P.nSend : 0;
#pragma unroll
      for (int i = 0; i < MP; i++) {
        a.recv[i] = P.recvFifo[i] + (uint64_t)rSlot[i] * P.slotBytes;
        a.recvFlag[i] = (uint32_t)(rs[i] + 1) & P.flagMask;  // NCCL_LL_FLAG(step + 1) under the rule
        a.send[i] = P.sendFifo[i] + (uint64_t)sSlot[i] * P.slotBytes;
        a.sendFlag[i] = (uint32_t)(ss[i] + 1) & P.flagMask;
      }
      a.srcIsInput = st.srcBuf == 0 && !P.firstWins;
      a.postOp = st.postOp && !P.firstWins;
      NEXR_TRACE(k, 1);
      bool arrived = true;
      for (uint64_t t = w; t < nTiles; t += G) {
        if constexpr (OP == nexrDevMinMax) {
          if ((a.redArg & 1) == 0) arrived &= ll_tile<D, OP, true, LLStepArgs, MP>(a, t, nBytes, nLines);
          else arrived &= ll_tile<D, OP, false, LLStepArgs, MP>(a, t, nBytes, nLines);
        } else {
          arrived &= ll_tile<D, OP, false, LLStepArgs, MP>(a, t, nBytes, nLines);
        }
      }
      NEXR_TRACE(k, 2);
      // a line never came: status set, this wave stops (its lines only; the other waves' are theirs)
      if (__builtin_amdgcn_ballot_w64(!arrived)) return;
      NEXR_TRACE(k, 3);
    }
    if (st.recv) {  // postRecv: the wave has used what it read of the step (its values are in the
      // outputs), so the sender may rewrite those lines. Relaxed: a release would also wait for the
      // outputs' own stores.
      if (lead)
        for (int i = 0; i < P.nRecv; i++)
          __hip_atomic_store(head_word(P.recvHead[i], w), rs[i] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
      for (int i = 0; i < MP; i++) {
        rs[i]++;
        rSlot[i] = rSlot[i] + 1 == (uint32_t)P.nSlots ? 0 : rSlot[i] + 1;
      }
    }
    if (st.send) {
#pragma unroll
      for (int j = 0; j < MP; j++) {
        ss[j]++;
        sSlot[j] = sSlot[j] + 1 == (uint32_t)P.nSlots ? 0 : sSlot[j] + 1;
      }
    }
    NEXR_TRACE(k, 4);
  }
  // incSend's cleanup (prims_ll.h:85-93). The host ends a launch at a cleaning send step and names the
  // send connections that clean there (P.cleanLast, bit j), so the step loop above carries nothing for
  // it: inside the loop the block cost C1's LL leg 5-10 % (its scalar registers are spilled already).
  // Every workgroup that owns a line of the SLOT writes here, not only those that own a data line, and
  // the grid is one workgroup per tile of a slot (at most kLLStepsMaxGrid), so that is every workgroup
  // of the launch: each wave waits for its own credit of the step (waitSend; the waves that moved data
  // have it cached) and then writes the clean lines it owns under ll_tile's map.
  if (P.cleanLast) {
    const uint64_t nLines = ((uint64_t)P.step[P.nSteps - 1].nElts * esz + 7) / 8;
#pragma unroll
    for (int j = 0; j < MP; j++) {
      if (!(P.cleanLast >> j & 1)) continue;
      // The step's send counter comes from the host, and the head is read afresh, so that nothing of the
      // loop's state lives on behind it (its registers are the parent's).
      const uint64_t s = P.cleanStep[j];
      const uint32_t slot = (uint32_t)(s % (uint64_t)P.nSlots);
      uint64_t head = 0;
      if (s + 1 > (uint64_t)P.nSlots &&
          !wait_head(head_word(const_cast<uint64_t*>(P.sendHead[j]), w), s + 1 - P.nSlots, head, P.timeoutTicks,
                     P.status))
        return;  // no credit: status set, this wave stops
      ll_clean_tiles(P.sendFifo[j] + (uint64_t)slot * P.slotBytes, (uint32_t)(s + 1) & P.flagMask, nLines,
                     P.slotBytes / 16, w, G);
    }
  }
#ifdef NEXR_LL_STEPS_TRACE
  if (threadIdx.x == 0)
    for (int k = 0; k < P.nSteps; k++)
      for (int j = 0; j < 5; j++) P.trace[((size_t)w * kLLStepsMax + k) * 5 + j] = tr[k][j];
#endif
#undef NEXR_TRACE
}

template <int D>
static hipError_t launch_ll_steps_dt(const LLStepsParams& a, int op, int grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (op) {
    case nexrDevSum: fn = (const void*)&reduce_copy_ll_steps_kernel<D, nexrDevSum>; break;
    case nexrDevProd: fn = (const void*)&reduce_copy_ll_steps_kernel<D, nexrDevProd>; break;
    case nexrDevMinMax: fn = (const void*)&reduce_copy_ll_steps_kernel<D, nexrDevMinMax>; break;
    case nexrDevPreMulSum: fn = (const void*)&reduce_copy_ll_steps_kernel<D, nexrDevPreMulSum>; break;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) fn = (const void*)&reduce_copy_ll_steps_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<LLStepsParams*>(&a)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_ll_steps(int dt, const LLStepsParams& a, int op, int grid, hipStream_t s) {
  switch (dt) {
    case nexrInt8: return launch_ll_steps_dt<nexrInt8>(a, op, grid, s);
    case nexrUint8: return launch_ll_steps_dt<nexrUint8>(a, op, grid, s);
    case nexrInt32: return launch_ll_steps_dt<nexrInt32>(a, op, grid, s);
    case nexrUint32: return launch_ll_steps_dt<nexrUint32>(a, op, grid, s);
    case nexrInt64: return launch_ll_steps_dt<nexrInt64>(a, op, grid, s);
    case nexrUint64: return launch_ll_steps_dt<nexrUint64>(a, op, grid, s);
    case nexrFloat16: return launch_ll_steps_dt<nexrFloat16>(a, op, grid, s);
    case nexrFloat32: return launch_ll_steps_dt<nexrFloat32>(a, op, grid, s);
    case nexrFloat64: return launch_ll_steps_dt<nexrFloat64>(a, op, grid, s);
    case nexrBfloat16: return launch_ll_steps_dt<nexrBfloat16>(a, op, grid, s);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// The runs of several Primitives in ONE launch (nexrReduceCopyLLStepsGroup): the step loop above for
// nMembers parameter blocks at once. Workgroup b runs member b / G as that member's workgroup b % G, so
// both ends of a connection between two members sit in the same grid: no second stream or hardware
// queue, and once the host has checked that nMembers * G workgroups are resident together, every poll's
// producer is running. The blocks (about 3.2 KiB each) do not fit the 4 KiB argument segment; they come
// from a table in device memory that nothing writes while the launch runs, read through the constant
// address space with a wave-uniform member index, so a step's record still arrives by scalar loads.
// All members report into one status word: one member's timeout ends the others' polls (ll_aborted).
// ---------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) LLStepsParams c_LLStepsParams;
typedef const __attribute__((address_space(4))) nexrLLStep c_LLStep;

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_ll_group_kernel(const LLStepsParams* table, int nMembers, int G) {
  constexpr uint64_t esz = 16 / Ty<D>::EPP;
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  const uint32_t m = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)G);
  const uint32_t w = blockIdx.x - m * (uint32_t)G;
  if (m >= (uint32_t)nMembers) return;
  c_LLStepsParams& P = ((c_LLStepsParams*)table)[m];
  const bool lead = (threadIdx.x & 63) == 0;
  const int nSlots = P.nSlots, nRecv = P.nRecv, nSend = P.nSend, nSteps = P.nSteps;
  const uint64_t slotBytes = P.slotBytes, timeoutTicks = P.timeoutTicks;
  const uint32_t flagMask = P.flagMask;
  uint32_t* const status = P.status;
  uint64_t rs[MP], ss[MP], headCache[MP];
  uint32_t rSlot[MP], sSlot[MP];
#pragma unroll
  for (int i = 0; i < MP; i++) {
    rs[i] = P.recvStep[i], ss[i] = P.sendStep[i], headCache[i] = 0;
    rSlot[i] = (uint32_t)(rs[i] % (uint64_t)nSlots), sSlot[i] = (uint32_t)(ss[i] % (uint64_t)nSlots);
  }
  // Every earlier launch of this stream has completed: whatever ran them, the slots before recvStep are read.
  if (lead)
    for (int i = 0; i < nRecv; i++)
      __hip_atomic_store(head_word(P.recvHead[i], w), rs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  LLStepArgs a;
  a.redArg = P.redArg;
  a.status = status;
  a.timeoutTicks = timeoutTicks;
  a.firstWins = P.firstWins;
  for (int k = 0; k < nSteps; k++) {
    c_LLStep& st = P.step[k];  // scalar loads from the table
    const uint64_t nBytes = (uint64_t)st.nElts * esz;
    const uint64_t nLines = (nBytes + 7) / 8;
    const uint64_t nTiles = (nLines + kLLTileLines - 1) / kLLTileLines;
    const bool stRecv = st.recv, stSend = st.send;
    if (w < nTiles) {
      if (stSend) {  // waitSend: the receiver's wave has read the step nSlots back
#pragma unroll
        for (int j = 0; j < MP; j++)
          if (j < nSend && ss[j] + 1 > (uint64_t)nSlots &&
              !wait_head(head_word(const_cast<uint64_t*>(P.sendHead[j]), w), ss[j] + 1 - nSlots, headCache[j],
                         timeoutTicks, status))
            return;  // no credit: status set, this wave stops
      }
      const int srcBuf = st.srcBuf, dstBuf = st.dstBuf;
      a.src = srcBuf == 0 ? P.input + st.srcIx * esz : srcBuf == 1 ? P.output + st.srcIx * esz : nullptr;
      a.dst = dstBuf == 0 ? const_cast<char*>(P.input) + st.dstIx * esz
              : dstBuf == 1 ? P.output + st.dstIx * esz : nullptr;
      a.nRecv = stRecv ? nRecv : 0;
      a.nSend = stSend ? nSend : 0;
#pragma unroll
      for (int i = 0; i < MP; i++) {
        a.recv[i] = P.recvFifo[i] + (uint64_t)rSlot[i] * slotBytes;
        a.recvFlag[i] = (uint32_t)(rs[i] + 1) & flagMask;  // NCCL_LL_FLAG(step + 1) under the rule
        a.send[i] = P.sendFifo[i] + (uint64_t)sSlot[i] * slotBytes;
        a.sendFlag[i] = (uint32_t)(ss[i] + 1) & flagMask;
      }
      a.srcIsInput = srcBuf == 0 && !a.firstWins;
      a.postOp = st.postOp && !a.firstWins;
      bool arrived = true;
      for (uint64_t t = w; t < nTiles; t += G) {
        if constexpr (OP == nexrDevMinMax) {
          if ((a.redArg & 1) == 0) arrived &= ll_tile<D, OP, true, LLStepArgs, MP>(a, t, nBytes, nLines);
          else arrived &= ll_tile<D, OP, false, LLStepArgs, MP>(a, t, nBytes, nLines);
        } else {
          arrived &= ll_tile<D, OP, false, LLStepArgs, MP>(a, t, nBytes, nLines);
        }
      }
      // a line never came: status set, this wave stops (its lines only; the other waves' are theirs)
      if (__builtin_amdgcn_ballot_w64(!arrived)) return;
    }
    if (stRecv) {  // postRecv, relaxed as in the single-member kernel
      if (lead)
        for (int i = 0; i < nRecv; i++)
          __hip_atomic_store(head_word(P.recvHead[i], w), rs[i] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
      for (int i = 0; i < MP; i++) {
        rs[i]++;
        rSlot[i] = rSlot[i] + 1 == (uint32_t)nSlots ? 0 : rSlot[i] + 1;
      }
    }
    if (stSend) {
#pragma unroll
      for (int j = 0; j < MP; j++) {
        ss[j]++;
        sSlot[j] = sSlot[j] + 1 == (uint32_t)nSlots ? 0 : sSlot[j] + 1;
      }
    }
  }
  // incSend's cleanup behind the member's last step, as in the single-member kernel: the host cuts every
  // member's launch at a cleaning send step and names the connections that clean there.
  const uint32_t cleanLast = P.cleanLast;
  if (cleanLast) {
    const uint64_t nLines = ((uint64_t)P.step[nSteps - 1].nElts * esz + 7) / 8;
#pragma unroll
    for (int j = 0; j < MP; j++) {
      if (!(cleanLast >> j & 1)) continue;
      const uint64_t s = P.cleanStep[j];
      const uint32_t slot = (uint32_t)(s % (uint64_t)nSlots);
      uint64_t head = 0;
      if (s + 1 > (uint64_t)nSlots &&
          !wait_head(head_word(const_cast<uint64_t*>(P.sendHead[j]), w), s + 1 - nSlots, head, timeoutTicks, status))
        return;  // no credit: status set, this wave stops
      ll_clean_tiles(P.sendFifo[j] + (uint64_t)slot * slotBytes, (uint32_t)(s + 1) & flagMask, nLines, slotBytes / 16,
                     w, G);
    }
  }
}

template <int D>
static const void* ll_group_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&reduce_copy_ll_group_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&reduce_copy_ll_group_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&reduce_copy_ll_group_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&reduce_copy_ll_group_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&reduce_copy_ll_group_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

static const void* ll_group_fn(int dt, int op) {
  switch (dt) {
    case nexrInt8: return ll_group_fn_dt<nexrInt8>(op);
    case nexrUint8: return ll_group_fn_dt<nexrUint8>(op);
    case nexrInt32: return ll_group_fn_dt<nexrInt32>(op);
    case nexrUint32: return ll_group_fn_dt<nexrUint32>(op);
    case nexrInt64: return ll_group_fn_dt<nexrInt64>(op);
    case nexrUint64: return ll_group_fn_dt<nexrUint64>(op);
    case nexrFloat16: return ll_group_fn_dt<nexrFloat16>(op);
    case nexrFloat32: return ll_group_fn_dt<nexrFloat32>(op);
    case nexrFloat64: return ll_group_fn_dt<nexrFloat64>(op);
    case nexrBfloat16: return ll_group_fn_dt<nexrBfloat16>(op);
  }
  return nullptr;
}

hipError_t launch_ll_group(int dt, int op, const LLStepsParams* table, int nMembers, int G, hipStream_t s) {
  const void* fn = ll_group_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {&table, &nMembers, &G};
  return hipLaunchKernel(fn, dim3((unsigned)(nMembers * G)), dim3(kBlock), args, 0, s);
}

// Workgroups of the group kernel one CU keeps resident (the registers decide: no LDS).
hipError_t ll_group_blocks_per_cu(int dt, int op, int* blocks) {
  const void* fn = ll_group_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, kBlock, 0);
}

// ---------------------------------------------------------------------------------------------
// LL128 (reference src/device/prims_ll128.h:86-331). The reference moves a 2 KiB wire slice per
// warp-32: lane wid holds regs[2g..2g+1] = user 16-B chunk ix(g, wid) = g*32 - 4*(g/2) + wid -
// (g%2)*(wid/8) and sends them as wire words 64g + 2wid (+1); lanes wid%8 == 7 carry the line flag
// in their odd word and therefore only half a chunk per g (the other half moved to g+1 by
// loadRegsFinish). Here one lane owns one 16-byte wire UNIT q = 32g + wid of a slice and derives
// which user bytes it carries from that same map, so the wire is byte-identical to the reference's
// while the kernel itself is laid out for 64-wide waves (any number of slices per workgroup).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool wait_flag64(const char* p, uint64_t flag, uint64_t timeoutTicks, uint32_t* status) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (ld_sys(p) != flag) {
    if (__builtin_amdgcn_s_memrealtime() - t0 > timeoutTicks) {
      if (status) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  return true;
}

// One tile = kLL128U sub-tiles of 256 wire units (two whole slices each); lane t owns unit t of
// every sub-tile, whose wire bytes sit at its unit index * 16, so each wave instruction moves 1 KiB
// of contiguous wire. A line's flag is the upper half of its unit 7, read by lane t | 7 in the same
// load; the other lanes of the line take it from there by a cross-lane read (the reference's warp
// vote over flag threads, prims_ll128.h:100-121). A lane's position in its slice (and so its user
// bytes, ix(g, wid)) is the same in every sub-tile.

template <int D, int OP, bool IsMin>
__device__ __forceinline__ void ll128_tile(const LL128Params& a, uint64_t tile, uint64_t nBytes, uint64_t nUnits) {
  using T = Ty<D>;
  using V = typename T::V;
  const uint64_t u0 = tile * kLL128TileUnits;
  const uint32_t tileUnits = (uint32_t)(nUnits - u0 < (uint64_t)kLL128TileUnits ? nUnits - u0 : kLL128TileUnits);
  const int q = (int)(threadIdx.x & 127);
  const int g = q >> 5, wid = q & 31;
  const bool flagLane = (wid & 7) == 7;
  uint64_t off, len;
  if (!flagLane) {
    off = (uint64_t)(g * 32 - 4 * (g / 2) + wid - (g % 2) * (wid / 8)) * 16;
    len = 16;
  } else {
    const int ge = g & ~1;  // the chunk loaded at the even g; odd g carries its second half
    off = (uint64_t)(ge * 32 - 4 * (ge / 2) + wid) * 16 + (g & 1) * 8;
    len = 8;
  }
  const int flagSrc = (int)((threadIdx.x & 63) | 7);
  u32x4 d[kLL128U];
  uint64_t valid[kLL128U], dOff[kLL128U];
  bool ok[kLL128U];
#pragma unroll
  for (int u = 0; u < kLL128U; u++) {
    const uint32_t m = u * kBlock + threadIdx.x;
    ok[u] = m < tileUnits;
    const uint64_t dBase = ((u0 + m) >> 7) * kLL128SliceData;
    const uint64_t eltBytes = !ok[u] ? 0 : nBytes - dBase < kLL128SliceData ? nBytes - dBase : kLL128SliceData;
    valid[u] = off < eltBytes ? (eltBytes - off < len ? eltBytes - off : len) : 0;
    dOff[u] = dBase + off;
    d[u] = (u32x4)0u;
    if (a.src) {
      if (valid[u] == 16) d[u] = *(const g_cu32x4_a1*)(a.src + dOff[u]);
      else if (valid[u]) d[u] = ld_partial(a.src + dOff[u], valid[u]);
      if constexpr (OP == nexrDevPreMulSum) {
        if (a.srcIsInput) d[u] = bc<u32x4>(T::mul(bc<V>(d[u]), T::splat(a.redArg)));
      }
    }
  }
  for (int i = 0; i < NEXR_MAX_SRCS; i++) {
    if (i >= a.nRecv) break;
    const auto r = wire_rsrc(a.recv[i] + u0 * 16, (uint64_t)tileUnits * 16);
    u32x4 x[kLL128U];
#pragma unroll
    for (int u = 0; u < kLL128U; u++) x[u] = wire_ld(r, (u * kBlock + threadIdx.x) * 16);  // past the end: zeros
    const uint64_t f = a.recvFlag[i];
#pragma unroll
    for (int u = 0; u < kLL128U; u++) {
      const uint32_t fl = __shfl(x[u].z, flagSrc), fh = __shfl(x[u].w, flagSrc);
      if (!__all(!ok[u] || (((uint64_t)fh << 32) | fl) == f) && ok[u]) {
        // not there yet: wait for this line's flag, then re-read the unit (readLL128's reload loop)
        const char* unitp = a.recv[i] + (u0 + u * kBlock + threadIdx.x) * 16;
        const char* flagp = a.recv[i] + (u0 + u * kBlock + (threadIdx.x | 7)) * 16 + 8;
        if (!wait_flag64(flagp, f, a.timeoutTicks, a.status)) {
          ok[u] = false;
        } else {
          const uint64_t lo = ld_sys(unitp), hi = ld_sys(unitp + 8);
          x[u] = (u32x4){(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
        }
      }
      if ((i == 0 && !a.src) || a.firstWins) d[u] = x[u];
      else d[u] = bc<u32x4>(reduce_step<D, OP, IsMin>(bc<V>(x[u]), bc<V>(d[u])));
    }
  }
#pragma unroll
  for (int u = 0; u < kLL128U; u++) {
    if constexpr (OP == nexrDevSumPostDiv) {
      if (a.postOp) d[u] = bc<u32x4>(T::divide(bc<V>(d[u]), a.redArg));
    }
    if constexpr (T::kCanon) {
      const bool arith = !a.firstWins && ((a.nRecv >= 1 && a.src) || a.nRecv >= 2 ||
                                          (OP == nexrDevPreMulSum && a.src && a.srcIsInput));
      if (arith) d[u] = bc<u32x4>(T::canon(bc<V>(d[u])));
    }
  }
  for (int i = 0; i < NEXR_MAX_DSTS; i++) {
    if (i >= a.nSend) break;
    const auto r = wire_rsrc(a.send[i] + u0 * 16, (uint64_t)tileUnits * 16);
    const uint64_t f = a.sendFlag[i];
#pragma unroll
    for (int u = 0; u < kLL128U; u++)
      if (ok[u])
        wire_st(r, (u * kBlock + threadIdx.x) * 16,
                flagLane ? (u32x4){d[u].x, d[u].y, (uint32_t)f, (uint32_t)(f >> 32)} : d[u]);
  }
  if (a.dst) {
#pragma unroll
    for (int u = 0; u < kLL128U; u++) {
      if (!ok[u] || !valid[u]) continue;
      if (valid[u] == 16) *(g_u32x4_a1*)(a.dst + dOff[u]) = d[u];
      else st_partial(a.dst + dOff[u], valid[u], d[u]);
    }
  }
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_ll128_kernel(LL128Params a) {
  const uint64_t nBytes = a.nElts * (16 / Ty<D>::EPP);
  const uint64_t nUnits = (nBytes + kLL128SliceData - 1) / kLL128SliceData * 128;
  const uint64_t nTiles = (nUnits + kLL128TileUnits - 1) / kLL128TileUnits;
  for (uint64_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
    if constexpr (OP == nexrDevMinMax) {
      if ((a.redArg & 1) == 0) ll128_tile<D, OP, true>(a, t, nBytes, nUnits);
      else ll128_tile<D, OP, false>(a, t, nBytes, nUnits);
    } else {
      ll128_tile<D, OP, false>(a, t, nBytes, nUnits);
    }
  }
}

template <int D>
static hipError_t launch_ll128_dt(const LL128Params& a, int op, int grid, hipStream_t s) {
  const void* fn = nullptr;
  switch (op) {
    case nexrDevSum: fn = (const void*)&reduce_copy_ll128_kernel<D, nexrDevSum>; break;
    case nexrDevProd: fn = (const void*)&reduce_copy_ll128_kernel<D, nexrDevProd>; break;
    case nexrDevMinMax: fn = (const void*)&reduce_copy_ll128_kernel<D, nexrDevMinMax>; break;
    case nexrDevPreMulSum: fn = (const void*)&reduce_copy_ll128_kernel<D, nexrDevPreMulSum>; break;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) fn = (const void*)&reduce_copy_ll128_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {const_cast<LL128Params*>(&a)};
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

hipError_t launch_ll128(int dt, const LL128Params& a, int op, int grid, hipStream_t s) {
  switch (dt) {
    case nexrInt8: return launch_ll128_dt<nexrInt8>(a, op, grid, s);
    case nexrUint8: return launch_ll128_dt<nexrUint8>(a, op, grid, s);
    case nexrInt32: return launch_ll128_dt<nexrInt32>(a, op, grid, s);
    case nexrUint32: return launch_ll128_dt<nexrUint32>(a, op, grid, s);
    case nexrInt64: return launch_ll128_dt<nexrInt64>(a, op, grid, s);
    case nexrUint64: return launch_ll128_dt<nexrUint64>(a, op, grid, s);
    case nexrFloat16: return launch_ll128_dt<nexrFloat16>(a, op, grid, s);
    case nexrFloat32: return launch_ll128_dt<nexrFloat32>(a, op, grid, s);
    case nexrFloat64: return launch_ll128_dt<nexrFloat64>(a, op, grid, s);
    case nexrBfloat16: return launch_ll128_dt<nexrBfloat16>(a, op, grid, s);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// LL128 step lists of several Primitives in ONE launch (nexrReduceCopyLL128StepsGroup): the group
// kernel's walk (workgroup b runs member b / G as its workgroup b % G; credits per wave on the device
// head words, waitSend / postRecv, prims_ll128.h:58-75) over LL128 steps whose hand-off is ordered by
// construction. The single step above accepts a line's data units from the very load that returned its
// flag, which is only right when the producer's kernel has completed: a line has ONE flag per 128 bytes
// and only 16-byte granules are observed untorn here, where the reference leans on NVIDIA's 128-byte
// warp store (prims_ll128.h:186-204, :278-285). Here instead:
//   producer, per wave: the seven data units of each of its lines (sc0 sc1), for every send connection;
//     then ONE s_waitcnt vmcnt(0); then the flag units (8 data bytes and the 64-bit flag, one 16-byte
//     store). The wave that stores a line's data stores its flag too, so no workgroup barrier.
//   consumer, per wave: polls its eight lines' flag units until all carry the step's flag, then loads
//     every unit AGAIN: a data unit enters the arithmetic only from a load issued after a load that
//     returned its line's flag had completed. The flag lane's own 8 data bytes share the flag's 16-byte
//     granule (the same observed 16-byte atomicity the LL lines rest on).
// Lane t owns unit t of a 256-unit sub-tile, so wave v owns units [64v, 64v + 64), eight whole lines: a
// line never spans waves, and the credit is per wave exactly as in the LL runs. No flag rule and no
// cleanup: the flags are 64-bit and the reference cleans nothing for LL128.
// ---------------------------------------------------------------------------------------------
struct LL128StepArgs {  // one step of a member's list, built in registers
  const char* src;
  char* dst;
  const char* recv[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t recvFlag[NEXR_LL_STEPS_MAX_PEERS];
  char* send[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t sendFlag[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t redArg;
  uint32_t* status;
  uint64_t timeoutTicks;
  int nRecv, nSend, srcIsInput, postOp, firstWins;
};

// Returns false when one of this wave's lines never arrived (status set or seen set; the wave's outputs
// of the tile stay unwritten). Every condition of the polls is wave-uniform: a tile holds whole slices
// (128 units), so a wave's 64 units are all inside it or all outside.
template <int D, int OP, bool IsMin>
__device__ __forceinline__ bool ll128_step_tile(const LL128StepArgs& a, uint64_t tile, uint64_t nBytes,
                                                uint64_t nUnits) {
  using T = Ty<D>;
  using V = typename T::V;
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  const uint64_t u0 = tile * kLL128TileUnits;
  const uint32_t tileUnits = (uint32_t)(nUnits - u0 < (uint64_t)kLL128TileUnits ? nUnits - u0 : kLL128TileUnits);
  const int q = (int)(threadIdx.x & 127);
  const int g = q >> 5, wid = q & 31;
  const bool flagLane = (wid & 7) == 7;
  uint64_t off, len;  // the lane's user bytes in its slice: ix(g, wid), as ll128_tile
  if (!flagLane) {
    off = (uint64_t)(g * 32 - 4 * (g / 2) + wid - (g % 2) * (wid / 8)) * 16;
    len = 16;
  } else {
    const int ge = g & ~1;
    off = (uint64_t)(ge * 32 - 4 * (ge / 2) + wid) * 16 + (g & 1) * 8;
    len = 8;
  }
  const int flagSrc = (int)((threadIdx.x & 63) | 7);
  u32x4 d[kLL128U];
  uint64_t valid[kLL128U], dOff[kLL128U];
  bool ok[kLL128U];
#pragma unroll
  for (int u = 0; u < kLL128U; u++) {
    const uint32_t m = u * kBlock + threadIdx.x;
    ok[u] = m < tileUnits;
    const uint64_t dBase = ((u0 + m) >> 7) * kLL128SliceData;
    const uint64_t eltBytes = !ok[u] ? 0 : nBytes - dBase < kLL128SliceData ? nBytes - dBase : kLL128SliceData;
    valid[u] = off < eltBytes ? (eltBytes - off < len ? eltBytes - off : len) : 0;
    dOff[u] = dBase + off;
    d[u] = (u32x4)0u;
    if (a.src) {
      if (valid[u] == 16) d[u] = *(const g_cu32x4_a1*)(a.src + dOff[u]);
      else if (valid[u]) d[u] = ld_partial(a.src + dOff[u], valid[u]);
      if constexpr (OP == nexrDevPreMulSum) {
        if (a.srcIsInput) d[u] = bc<u32x4>(T::mul(bc<V>(d[u]), T::splat(a.redArg)));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MP; i++) {
    if (i >= a.nRecv) break;
    const auto r = wire_rsrc(a.recv[i] + u0 * 16, (uint64_t)tileUnits * 16);
    const uint64_t f = a.recvFlag[i];
#pragma unroll
    for (int u = 0; u < kLL128U; u++) {
      if (!__builtin_amdgcn_ballot_w64(ok[u])) continue;  // none of this wave's units in the tile
      const uint32_t o = (u * kBlock + threadIdx.x) * 16;
      // The poll (readLL128's flag vote, prims_ll128.h:100-121): relaxed, bounded, and what it returns
      // beside the flags is thrown away.
      uint64_t t0 = 0;
      for (uint32_t tries = 1;; tries++) {
        const u32x4 p = wire_ld(r, o);  // past the end: zeros
        const uint32_t fl = __shfl(p.z, flagSrc), fh = __shfl(p.w, flagSrc);
        if (__all(!ok[u] || (((uint64_t)fh << 32) | fl) == f)) break;
        if (tries % kLLAbortEvery == 0 && ll_aborted(a.status)) return false;  // checkAbort (primitives.h:142-156)
        if (tries % kLLClockEvery == 0) {
          const uint64_t now = __builtin_amdgcn_s_memrealtime();
          if (!t0) t0 = now;
          else if (now - t0 > a.timeoutTicks) {
            if (a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
          }
        }
        __builtin_amdgcn_s_sleep(1);
      }
      // Every line's flag came back in a load that has completed (its value was branched on): the loads
      // from here on are issued behind it. The wait keeps them there whatever the compiler would do.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const u32x4 x = wire_ld(r, o);
      if ((i == 0 && !a.src) || a.firstWins) d[u] = x;
      else d[u] = bc<u32x4>(reduce_step<D, OP, IsMin>(bc<V>(x), bc<V>(d[u])));
    }
  }
#pragma unroll
  for (int u = 0; u < kLL128U; u++) {
    if constexpr (OP == nexrDevSumPostDiv) {
      if (a.postOp) d[u] = bc<u32x4>(T::divide(bc<V>(d[u]), a.redArg));
    }
    if constexpr (T::kCanon) {
      const bool arith = !a.firstWins && ((a.nRecv >= 1 && a.src) || a.nRecv >= 2 ||
                                          (OP == nexrDevPreMulSum && a.src && a.srcIsInput));
      if (arith) d[u] = bc<u32x4>(T::canon(bc<V>(d[u])));
    }
  }
  if (a.nSend > 0) {
    // data units, one drain for every send connection of the step, then the flag units
#pragma unroll
    for (int i = 0; i < MP; i++) {
      if (i >= a.nSend) break;
      const auto r = wire_rsrc(a.send[i] + u0 * 16, (uint64_t)tileUnits * 16);
#pragma unroll
      for (int u = 0; u < kLL128U; u++)
        if (ok[u] && !flagLane) wire_st(r, (u * kBlock + threadIdx.x) * 16, d[u]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < MP; i++) {
      if (i >= a.nSend) break;
      const auto r = wire_rsrc(a.send[i] + u0 * 16, (uint64_t)tileUnits * 16);
      const uint64_t f = a.sendFlag[i];
#pragma unroll
      for (int u = 0; u < kLL128U; u++)
        if (ok[u] && flagLane)
          wire_st(r, (u * kBlock + threadIdx.x) * 16, (u32x4){d[u].x, d[u].y, (uint32_t)f, (uint32_t)(f >> 32)});
    }
  }
  if (a.dst) {
#pragma unroll
    for (int u = 0; u < kLL128U; u++) {
      if (!ok[u] || !valid[u]) continue;
      if (valid[u] == 16) *(g_u32x4_a1*)(a.dst + dOff[u]) = d[u];
      else st_partial(a.dst + dOff[u], valid[u], d[u]);
    }
  }
  return true;
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_ll128_group_kernel(const LLStepsParams* table, int nMembers,
                                                                         int G) {
  constexpr uint64_t esz = 16 / Ty<D>::EPP;
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  const uint32_t m = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)G);
  const uint32_t w = blockIdx.x - m * (uint32_t)G;
  if (m >= (uint32_t)nMembers) return;
  c_LLStepsParams& P = ((c_LLStepsParams*)table)[m];
  const bool lead = (threadIdx.x & 63) == 0;
  const int nSlots = P.nSlots, nRecv = P.nRecv, nSend = P.nSend, nSteps = P.nSteps;
  const uint64_t slotBytes = P.slotBytes, timeoutTicks = P.timeoutTicks;
  uint32_t* const status = P.status;
  uint64_t rs[MP], ss[MP], headCache[MP];
  uint32_t rSlot[MP], sSlot[MP];
#pragma unroll
  for (int i = 0; i < MP; i++) {
    rs[i] = P.recvStep[i], ss[i] = P.sendStep[i], headCache[i] = 0;
    rSlot[i] = (uint32_t)(rs[i] % (uint64_t)nSlots), sSlot[i] = (uint32_t)(ss[i] % (uint64_t)nSlots);
  }
  // Every earlier launch of this stream has completed: whatever ran them, the slots before recvStep are read.
  if (lead)
    for (int i = 0; i < nRecv; i++)
      __hip_atomic_store(head_word(P.recvHead[i], w), rs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  LL128StepArgs a;
  a.redArg = P.redArg;
  a.status = status;
  a.timeoutTicks = timeoutTicks;
  a.firstWins = P.firstWins;
  for (int k = 0; k < nSteps; k++) {
    c_LLStep& st = P.step[k];  // scalar loads from the table
    const uint64_t nBytes = (uint64_t)st.nElts * esz;
    const uint64_t nUnits = (nBytes + kLL128SliceData - 1) / kLL128SliceData * 128;
    const uint64_t nTiles = (nUnits + kLL128TileUnits - 1) / kLL128TileUnits;
    const bool stRecv = st.recv, stSend = st.send;
    if (w < nTiles) {
      if (stSend) {  // waitSend: the receiver's wave has read the step nSlots back
#pragma unroll
        for (int j = 0; j < MP; j++)
          if (j < nSend && ss[j] + 1 > (uint64_t)nSlots &&
              !wait_head(head_word(const_cast<uint64_t*>(P.sendHead[j]), w), ss[j] + 1 - nSlots, headCache[j],
                         timeoutTicks, status))
            return;  // no credit: status set, this wave stops
      }
      const int srcBuf = st.srcBuf, dstBuf = st.dstBuf;
      a.src = srcBuf == 0 ? P.input + st.srcIx * esz : srcBuf == 1 ? P.output + st.srcIx * esz : nullptr;
      a.dst = dstBuf == 0 ? const_cast<char*>(P.input) + st.dstIx * esz
              : dstBuf == 1 ? P.output + st.dstIx * esz : nullptr;
      a.nRecv = stRecv ? nRecv : 0;
      a.nSend = stSend ? nSend : 0;
#pragma unroll
      for (int i = 0; i < MP; i++) {
        a.recv[i] = P.recvFifo[i] + (uint64_t)rSlot[i] * slotBytes;
        a.recvFlag[i] = rs[i] + 1;  // the 64-bit flag: step + 1
        a.send[i] = P.sendFifo[i] + (uint64_t)sSlot[i] * slotBytes;
        a.sendFlag[i] = ss[i] + 1;
      }
      a.srcIsInput = srcBuf == 0 && !a.firstWins;
      a.postOp = st.postOp && !a.firstWins;
      for (uint64_t t = w; t < nTiles; t += G) {
        bool arrived;
        if constexpr (OP == nexrDevMinMax) {
          if ((a.redArg & 1) == 0) arrived = ll128_step_tile<D, OP, true>(a, t, nBytes, nUnits);
          else arrived = ll128_step_tile<D, OP, false>(a, t, nBytes, nUnits);
        } else {
          arrived = ll128_step_tile<D, OP, false>(a, t, nBytes, nUnits);
        }
        // a line never came: status set, this wave stops (its lines only; the other waves' are theirs)
        if (!arrived) return;
      }
    }
    if (stRecv) {  // postRecv, relaxed as in the LL runs: what the wave read is in its outputs
      if (lead)
        for (int i = 0; i < nRecv; i++)
          __hip_atomic_store(head_word(P.recvHead[i], w), rs[i] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
      for (int i = 0; i < MP; i++) {
        rs[i]++;
        rSlot[i] = rSlot[i] + 1 == (uint32_t)nSlots ? 0 : rSlot[i] + 1;
      }
    }
    if (stSend) {
#pragma unroll
      for (int j = 0; j < MP; j++) {
        ss[j]++;
        sSlot[j] = sSlot[j] + 1 == (uint32_t)nSlots ? 0 : sSlot[j] + 1;
      }
    }
  }
}

template <int D>
static const void* ll128_group_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&reduce_copy_ll128_group_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&reduce_copy_ll128_group_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&reduce_copy_ll128_group_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&reduce_copy_ll128_group_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&reduce_copy_ll128_group_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

static const void* ll128_group_fn(int dt, int op) {
  switch (dt) {
    case nexrInt8: return ll128_group_fn_dt<nexrInt8>(op);
    case nexrUint8: return ll128_group_fn_dt<nexrUint8>(op);
    case nexrInt32: return ll128_group_fn_dt<nexrInt32>(op);
    case nexrUint32: return ll128_group_fn_dt<nexrUint32>(op);
    case nexrInt64: return ll128_group_fn_dt<nexrInt64>(op);
    case nexrUint64: return ll128_group_fn_dt<nexrUint64>(op);
    case nexrFloat16: return ll128_group_fn_dt<nexrFloat16>(op);
    case nexrFloat32: return ll128_group_fn_dt<nexrFloat32>(op);
    case nexrFloat64: return ll128_group_fn_dt<nexrFloat64>(op);
    case nexrBfloat16: return ll128_group_fn_dt<nexrBfloat16>(op);
  }
  return nullptr;
}

hipError_t launch_ll128_group(int dt, int op, const LLStepsParams* table, int nMembers, int G, hipStream_t s) {
  const void* fn = ll128_group_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {&table, &nMembers, &G};
  return hipLaunchKernel(fn, dim3((unsigned)(nMembers * G)), dim3(kBlock), args, 0, s);
}

hipError_t ll128_group_blocks_per_cu(int dt, int op, int* blocks) {
  const void* fn = ll128_group_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, kBlock, 0);
}

}  // namespace nexr

// SIMPLE step lists in group launches: the same code object (tests/test_code_objects.py counts them).
#include "nexr_simple.hip"
// The symmetric all-reduce in one launch: the same code object again.
#include "nexr_sym.hip"
// The ring collectives in one launch with the ring's bytes: the same code object again.
#include "nexr_flat.hip"
#include "nexr_flat_tree.hip"
// Several of them in one launch (nexrFlatGroup): the same code object again.
#include "nexr_flat_group.hip"
