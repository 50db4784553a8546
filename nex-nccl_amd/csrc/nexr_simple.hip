// nexr_simple.hip — SIMPLE-protocol step lists of several Primitives in ONE launch
// (nexrReduceCopySimpleStepsGroup), for gfx950. Included at the end of nexr_ll.hip: the LL / LL128 object
// stays the one code object beside the per-datatype ones, and the status-word poll and the
// constant-address-space table reads are that file's.
//
// What a step record computes is one slice of genericOp (reference src/device/prims_simple.h:190-330,
// restated on the host in nexr_emu.h): srcs = [user src, the slot of every receive connection], dsts =
// [user dst, the slot of every send connection], acc = srcs[0] (the USER source first: nexrReduceCopy's
// order, not the LL kernels' peer-first one), the PreMulSum pre-op on source 0 when it is the user
// input, the post-op as the record says. SIMPLE data carries no flags: a slot is ordered by its
// connection's step counters alone (waitPeer / postPeer, prims_simple.h:111-188), which here are words in
// device memory, one tail word and one head word per workgroup and connection.
//
// Geometry. Tile t of a slice is bytes [t * 4096, t * 4096 + 4096) from the slice's start, lane l of the
// workgroup its 16-byte pack l; tile t belongs to workgroup t % G on both ends of every connection. A
// workgroup takes kSimpleU of its tiles at a time, all their K loads issued before the first fold.
//
// Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility, the always-valid form), system scope
// throughout as in the LL kernels:
//   producer: plain stores to the send slots; every wave s_waitcnt vmcnt(0); workgroup barrier; lane 0:
//     release fence, s_waitcnt vmcnt(0) (inline asm: the compiler may not drop it), relaxed atomic store
//     of the workgroup's tail word;
//   consumer: wave 0 polls the tail word (relaxed, s_sleep between tries, bounded in time), ONE acquire
//     fence, s_waitcnt vmcnt(0), its verdict into LDS, workgroup barrier, then everybody's plain loads.
// The head goes back once every wave's loads of the slot have returned (their s_waitcnt vmcnt(0) and
// the same barrier); the sender's wave 0 polls it before the workgroup stores into the slot again.
// A poll that times out (or finds the status word set) makes the whole workgroup leave, through the
// verdict word: no wave is left at a barrier.
//
// DirectWrite (nexrReduceCopySimpleStepsGroupDirect; prims_simple.h:148-164, :258-269) is a second kernel,
// reduce_copy_simple_group_direct_kernel, behind the first: the same waits, credits and posts, with a slice's
// receive source and send destinations in user memory where the record and the connection say so.

namespace nexr {

constexpr int kSimpleU = 4;  // tiles of a workgroup in flight
static_assert(kSimpleTileBytes == kBlock * 16, "one 16-byte pack per lane and tile");

typedef const __attribute__((address_space(4))) SimpleStepsParams c_SimpleStepsParams;

__device__ __forceinline__ uint64_t* credit_word(const uint64_t* base, uint32_t w) {
  return const_cast<uint64_t*>(base) + (size_t)w * (kSimpleCreditStride / 8);
}

// Wave 0's poll of one credit word, by every lane on the same word (one request). Relaxed; t0 is shared by
// the polls of one slice, so the slice as a whole is bounded by the timeout.
__device__ __forceinline__ bool simple_wait(const uint64_t* p, uint64_t need, uint64_t& t0, uint64_t timeoutTicks,
                                            uint32_t* status) {
  for (uint32_t tries = 1;; tries++) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= need) return true;
    if (tries % kLLAbortEvery == 0 && ll_aborted(status)) return false;
    const uint64_t now = __builtin_amdgcn_s_memrealtime();
    if (!t0) t0 = now;
    else if (now - t0 > timeoutTicks) {
      if (status) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

struct SimpleStepArgs {  // one slice of a member's list, built in registers
  const char* src;       // user source (nullable): source 0 when there
  char* dst;             // user destination (nullable)
  const char* recv[NEXR_LL_STEPS_MAX_PEERS];
  char* send[NEXR_LL_STEPS_MAX_PEERS];
  uint64_t redArg;
  int nFold;  // receive slots that enter the fold (shipped semantics: only source 0 does)
  int nSend, preOp, postOp;
};

// The first n (< 16) bytes at p as a zero-padded pack and the reverse, in rolled byte loops: a slice has at
// most one partial pack, so its code is kept small (ld_partial / st_partial of the LL kernels are unrolled).
__device__ __forceinline__ u32x4 ld_bytes(const char* p, uint32_t n) {
  uint64_t lo = 0, hi = 0;
#pragma unroll 1
  for (int b = (int)n - 1; b >= 0; b--) {
    const uint64_t x = (uint8_t)p[b];
    if (b >= 8) hi = (hi << 8) | x;
    else lo = (lo << 8) | x;
  }
  return (u32x4){(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}
__device__ __forceinline__ void st_bytes(char* p, uint32_t n, u32x4 v) {
  uint64_t lo = (uint64_t)v.y << 32 | v.x, hi = (uint64_t)v.w << 32 | v.z;
#pragma unroll 1
  for (uint32_t b = 0; b < n; b++) {
    if (b < 8) {
      p[b] = (char)lo;
      lo >>= 8;
    } else {
      p[b] = (char)hi;
      hi >>= 8;
    }
  }
}

// One position: acc = srcs[0] (the user source when there, with its pre-op), folded with the receive slots
// in order, the post-op, ncclFromFloat's NaN canonicalisation when any arithmetic ran (nexr_fold.hpp).
template <int D, int OP, bool IsMin>
__device__ __forceinline__ u32x4 simple_fold(const SimpleStepArgs& a, bool hasSrc, bool canon, u32x4 us,
                                             const u32x4 (&r)[NEXR_LL_STEPS_MAX_PEERS]) {
  using T = Ty<D>;
  using V = typename T::V;
  V acc;
  if (hasSrc) {
    acc = bc<V>(us);
    if constexpr (OP == nexrDevPreMulSum) {
      if (a.preOp) acc = T::mul(acc, T::splat(a.redArg));  // Apply_PreOp on source 0, the user input
    }
  } else {
    acc = bc<V>(r[0]);
  }
#pragma unroll
  for (int i = 0; i < NEXR_LL_STEPS_MAX_PEERS; i++)
    if (i < a.nFold && (i > 0 || hasSrc)) acc = reduce_step<D, OP, IsMin>(acc, bc<V>(r[i]));
  if constexpr (OP == nexrDevSumPostDiv) {
    if (a.postOp) acc = T::divide(acc, a.redArg);
  }
  if constexpr (T::kCanon) {
    if (canon) acc = T::canon(acc);
  }
  return bc<u32x4>(acc);
}

// The tiles of workgroup w of one slice: loads, fold, stores. User buffers at any alignment (unaligned
// 16-byte accesses); slots are 16-byte aligned. The slice's last, partial pack (nBytes % 16 bytes) is left
// to the lane that owns it, behind the loop: user bytes one at a time, the slot's pack loaded whole (it
// lies inside the slot) and stored by bytes, so that a slot holds exactly the slice's bytes.
//
// Direct (nexrReduceCopySimpleStepsGroupDirect): a receive source or a send destination may be user memory
// (the member's own output, a peer's output) in place of a slot, so those accesses are the unaligned ones too
// and the last partial pack of a receive source is loaded by bytes: it no longer lies inside a slot.
template <int D, int OP, bool IsMin, bool Direct = false>
__device__ __forceinline__ void simple_tiles(const SimpleStepArgs& a, uint32_t w, uint32_t G, uint64_t nBytes,
                                             uint64_t nTiles) {
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  using RecvPack = typename std::conditional<Direct, g_cu32x4_a1, g_cu32x4>::type;
  using SendPack = typename std::conditional<Direct, g_u32x4_a1, g_u32x4>::type;
  const bool hasSrc = a.src != nullptr;
  const bool canon = (hasSrc ? 1 : 0) + a.nFold >= 2 || (OP == nexrDevPreMulSum && a.preOp);
  const uint64_t fullBytes = nBytes & ~(uint64_t)15;
  for (uint64_t t0 = w; t0 < nTiles; t0 += (uint64_t)G * kSimpleU) {
    uint64_t off[kSimpleU];
    bool valid[kSimpleU];
    u32x4 us[kSimpleU], r[kSimpleU][MP];
#pragma unroll
    for (int u = 0; u < kSimpleU; u++) {
      off[u] = (t0 + (uint64_t)u * G) * kSimpleTileBytes + threadIdx.x * 16u;
      valid[u] = off[u] < fullBytes;  // a whole pack (tiles past the slice's end fail this too)
      us[u] = (u32x4)0u;
    }
    if (hasSrc) {
#pragma unroll
      for (int u = 0; u < kSimpleU; u++)
        if (valid[u]) us[u] = *(const g_cu32x4_a1*)(a.src + off[u]);
    }
#pragma unroll
    for (int i = 0; i < MP; i++) {
#pragma unroll
      for (int u = 0; u < kSimpleU; u++) {
        r[u][i] = (u32x4)0u;
        if (i < a.nFold && valid[u]) r[u][i] = *(const RecvPack*)(a.recv[i] + off[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kSimpleU; u++) {
      if (!valid[u]) continue;
      const u32x4 out = simple_fold<D, OP, IsMin>(a, hasSrc, canon, us[u], r[u]);
#pragma unroll
      for (int j = 0; j < MP; j++)
        if (j < a.nSend) *(SendPack*)(a.send[j] + off[u]) = out;
      if (a.dst) *(g_u32x4_a1*)(a.dst + off[u]) = out;
    }
  }
  const uint32_t rem = (uint32_t)(nBytes - fullBytes);
  if (rem) {
    const uint64_t tile = fullBytes / kSimpleTileBytes;
    if (tile % G == w && threadIdx.x == (uint32_t)(fullBytes % kSimpleTileBytes) / 16u) {
      u32x4 us = (u32x4)0u, r[MP];
      if (hasSrc) us = ld_bytes(a.src + fullBytes, rem);
#pragma unroll
      for (int i = 0; i < MP; i++) {
        r[i] = (u32x4)0u;
        if constexpr (Direct) {
          if (i < a.nFold) r[i] = ld_bytes(a.recv[i] + fullBytes, rem);
        } else {
          if (i < a.nFold) r[i] = *(const g_cu32x4*)(a.recv[i] + fullBytes);
        }
      }
      const u32x4 out = simple_fold<D, OP, IsMin>(a, hasSrc, canon, us, r);
#pragma unroll
      for (int j = 0; j < MP; j++)  // unrolled: a.send[] stays in registers
        if (j < a.nSend) st_bytes(a.send[j] + fullBytes, rem, out);
      if (a.dst) st_bytes(a.dst + fullBytes, rem, out);
    }
  }
}

template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_simple_group_kernel(const SimpleStepsParams* table, int nMembers,
                                                                          int G) {
  constexpr uint64_t esz = 16 / Ty<D>::EPP;
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  __shared__ uint32_t verdict;
  const uint32_t m = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)G);
  const uint32_t w = blockIdx.x - m * (uint32_t)G;
  if (m >= (uint32_t)nMembers) return;
  c_SimpleStepsParams& P = ((c_SimpleStepsParams*)table)[m];
  const bool lane0 = threadIdx.x == 0;
  const int nSlots = P.nSlots, nRecv = P.nRecv, nSend = P.nSend, nSteps = P.nSteps;
  const uint64_t sps = (uint64_t)P.stepPerSlice;
  const uint64_t slotBytes = P.slotBytes, timeoutTicks = P.timeoutTicks;
  uint32_t* const status = P.status;
  const int firstWins = P.firstWins;
  uint64_t rs[MP], ss[MP];
#pragma unroll
  for (int i = 0; i < MP; i++) rs[i] = P.recvStep[i], ss[i] = P.sendStep[i];
  // Every earlier launch of this stream has completed, whatever ran its steps: the slots before recvStep
  // are read and those before sendStep written. (The "return credits" store of a connection that host-
  // sequenced steps used before.)
  if (lane0) {
    for (int i = 0; i < nRecv; i++)
      __hip_atomic_store(credit_word(P.recvHead[i], w), rs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int j = 0; j < nSend; j++)
      __hip_atomic_store(credit_word(P.sendTail[j], w), ss[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  SimpleStepArgs a;
  a.redArg = P.redArg;
  for (int k = 0; k < nSteps; k++) {
    c_LLStep& st = P.step[k];  // scalar loads from the table
    const uint64_t nBytes = (uint64_t)st.nElts * esz;
    const uint64_t nTiles = (nBytes + kSimpleTileBytes - 1) / kSimpleTileBytes;
    const bool stRecv = st.recv, stSend = st.send;
    const bool owns = w < nTiles;  // workgroup-uniform, as everything the barriers below depend on
    if (owns) {
      if (stRecv || stSend) {
        if (threadIdx.x < 64) {
          bool ok = true;
          uint64_t t0 = 0;
#pragma unroll
          for (int i = 0; i < MP; i++)  // waitPeer, receive side: tail >= step + StepPerSlice
            if (ok && stRecv && i < nRecv)
              ok = simple_wait(credit_word(P.recvTail[i], w), rs[i] + sps, t0, timeoutTicks, status);
#pragma unroll
          for (int j = 0; j < MP; j++)  // send side: head + NCCL_STEPS >= step + StepPerSlice
            if (ok && stSend && j < nSend && ss[j] + sps > (uint64_t)nSlots)
              ok = simple_wait(credit_word(P.sendHead[j], w), ss[j] + sps - (uint64_t)nSlots, t0, timeoutTicks, status);
          if (stRecv) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed before the barrier
          }
          if (lane0) verdict = ok ? 1u : 0u;
        }
        __syncthreads();
        if (verdict == 0u) return;  // every wave of the workgroup: status is set, nothing of the slice is written
      }
      const int srcBuf = st.srcBuf, dstBuf = st.dstBuf;
      a.src = srcBuf == 0 ? P.input + st.srcIx * esz : srcBuf == 1 ? P.output + st.srcIx * esz : nullptr;
      a.dst = dstBuf == 0 ? const_cast<char*>(P.input) + st.dstIx * esz
              : dstBuf == 1 ? P.output + st.dstIx * esz : nullptr;
      // shipped semantics: every reduce returns acc = srcs[0], no pre-op, no post-op
      a.nFold = !stRecv ? 0 : !firstWins ? nRecv : a.src ? 0 : 1;
      a.nSend = stSend ? nSend : 0;
      a.preOp = srcBuf == 0 && !firstWins;
      a.postOp = st.postOp && !firstWins;
#pragma unroll
      for (int i = 0; i < MP; i++) {
        a.recv[i] = P.recvFifo[i] + (rs[i] % (uint64_t)nSlots) * slotBytes;
        a.send[i] = P.sendFifo[i] + (ss[i] % (uint64_t)nSlots) * slotBytes;
      }
      if constexpr (OP == nexrDevMinMax) {
        if ((a.redArg & 1) == 0) simple_tiles<D, OP, true>(a, w, (uint32_t)G, nBytes, nTiles);
        else simple_tiles<D, OP, false>(a, w, (uint32_t)G, nBytes, nTiles);
      } else {
        simple_tiles<D, OP, false>(a, w, (uint32_t)G, nBytes, nTiles);
      }
      if (stRecv || stSend) {
        // every wave: its stores to the send slots have completed and its loads of the receive slots returned
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
    // postPeer. A workgroup without a tile of the slice posts as well: nobody waits for it on this slice.
    if (lane0) {
      if (stSend) {
        if (owns) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-back has completed before the tail goes out
        }
        for (int j = 0; j < nSend; j++)
          __hip_atomic_store(credit_word(P.sendTail[j], w), ss[j] + sps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (stRecv)
        for (int i = 0; i < nRecv; i++)
          __hip_atomic_store(credit_word(P.recvHead[i], w), rs[i] + sps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (stRecv) {
#pragma unroll
      for (int i = 0; i < MP; i++) rs[i] += sps;
    }
    if (stSend) {
#pragma unroll
      for (int j = 0; j < MP; j++) ss[j] += sps;
    }
  }
}

// The kernel of nexrReduceCopySimpleStepsGroupDirect: reduce_copy_simple_group_kernel with DirectWrite ends.
// A kernel of its own, so that the FIFO-only kernels keep their code: the waits, the credits, the barriers and
// the posts are the same statements; what differs is where a slice's receive source and send destinations
// point, and the slice that moves nothing.
typedef const __attribute__((address_space(4))) SimpleDirectParams c_SimpleDirectParams;
template <int D, int OP>
__global__ __launch_bounds__(kBlock) void reduce_copy_simple_group_direct_kernel(const SimpleDirectParams* table,
                                                                                 int nMembers, int G) {
  constexpr uint64_t esz = 16 / Ty<D>::EPP;
  constexpr int MP = NEXR_LL_STEPS_MAX_PEERS;
  __shared__ uint32_t verdict;
  const uint32_t m = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)G);
  const uint32_t w = blockIdx.x - m * (uint32_t)G;
  if (m >= (uint32_t)nMembers) return;
  c_SimpleDirectParams& E = ((c_SimpleDirectParams*)table)[m];
  c_SimpleStepsParams& P = E;  // the FIFO-only entry is its base
  const bool lane0 = threadIdx.x == 0;
  const int nSlots = P.nSlots, nRecv = P.nRecv, nSend = P.nSend, nSteps = P.nSteps;
  const uint64_t sps = (uint64_t)P.stepPerSlice;
  const uint64_t slotBytes = P.slotBytes, timeoutTicks = P.timeoutTicks;
  uint32_t* const status = P.status;
  const int firstWins = P.firstWins;
  uint64_t rs[MP], ss[MP];
#pragma unroll
  for (int i = 0; i < MP; i++) rs[i] = P.recvStep[i], ss[i] = P.sendStep[i];
  // Every earlier launch of this stream has completed, whatever ran its steps: the slots before recvStep
  // are read and those before sendStep written. (The "return credits" store of a connection that host-
  // sequenced steps used before.)
  if (lane0) {
    for (int i = 0; i < nRecv; i++)
      __hip_atomic_store(credit_word(P.recvHead[i], w), rs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int j = 0; j < nSend; j++)
      __hip_atomic_store(credit_word(P.sendTail[j], w), ss[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  SimpleStepArgs a;
  a.redArg = P.redArg;
  for (int k = 0; k < nSteps; k++) {
    c_LLStep& st = P.step[k];  // scalar loads from the table
    const uint64_t nBytes = (uint64_t)st.nElts * esz;
    const uint64_t nTiles = (nBytes + kSimpleTileBytes - 1) / kSimpleTileBytes;
    const bool stRecv = st.recv, stSend = st.send;
    const bool owns = w < nTiles;  // workgroup-uniform, as everything the barriers below depend on
    if (owns) {
      if (stRecv || stSend) {
        if (threadIdx.x < 64) {
          bool ok = true;
          uint64_t t0 = 0;
#pragma unroll
          for (int i = 0; i < MP; i++)  // waitPeer, receive side: tail >= step + StepPerSlice
            if (ok && stRecv && i < nRecv)
              ok = simple_wait(credit_word(P.recvTail[i], w), rs[i] + sps, t0, timeoutTicks, status);
#pragma unroll
          for (int j = 0; j < MP; j++)  // send side: head + NCCL_STEPS >= step + StepPerSlice
            if (ok && stSend && j < nSend && ss[j] + sps > (uint64_t)nSlots)
              ok = simple_wait(credit_word(P.sendHead[j], w), ss[j] + sps - (uint64_t)nSlots, t0, timeoutTicks, status);
          if (stRecv) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed before the barrier
          }
          if (lane0) verdict = ok ? 1u : 0u;
        }
        __syncthreads();
        if (verdict == 0u) return;  // every wave of the workgroup: status is set, nothing of the slice is written
      }
      const int srcBuf = st.srcBuf, dstBuf = st.dstBuf;
      a.src = srcBuf == 0 ? P.input + st.srcIx * esz : srcBuf == 1 ? P.output + st.srcIx * esz : nullptr;
      a.dst = dstBuf == 0 ? const_cast<char*>(P.input) + st.dstIx * esz
              : dstBuf == 1 ? P.output + st.dstIx * esz : nullptr;
      // shipped semantics: every reduce returns acc = srcs[0], no pre-op, no post-op
      a.nFold = !stRecv ? 0 : !firstWins ? nRecv : a.src ? 0 : 1;
      a.nSend = stSend ? nSend : 0;
      a.preOp = srcBuf == 0 && !firstWins;
      a.postOp = st.postOp && !firstWins;
#pragma unroll
      for (int i = 0; i < MP; i++) {
        a.recv[i] = P.recvFifo[i] + (rs[i] % (uint64_t)nSlots) * slotBytes;
        a.send[i] = P.sendFifo[i] + (ss[i] % (uint64_t)nSlots) * slotBytes;
      }
      // waitPeer's DirectWrite pointers (prims_simple.h:148-164): an end is direct when the record permits it
      // (pad[0]) and the connection is (the table entry). Both ends compute dstIx * esz alike.
      const uint32_t bits = st.pad[0];
      const bool dRecv = stRecv && (bits & NEXR_SIMPLE_DIRECT_RECV) && E.recvDirect;
      if (dRecv) a.recv[0] = P.output + st.dstIx * esz;
      if (bits & NEXR_SIMPLE_DIRECT_SEND) {
#pragma unroll
        for (int j = 0; j < MP; j++)
          if (E.sendDirect[j]) a.send[j] = E.sendDirect[j] + st.dstIx * esz;
      }
      // :258-269: source 0 IS the user destination. Nothing goes to the output; a sending record copies the one
      // source to its send destinations bit for bit (directRecvCopyDirectSend), any other moves no data
      // (directRecv): it has waited, and advances and posts below.
      bool moves = true;
      if (dRecv && srcBuf == -1 && dstBuf == 1) {
        a.dst = nullptr;
        a.postOp = 0;
        moves = stSend;
      }
      if (moves) {
        if constexpr (OP == nexrDevMinMax) {
          if ((a.redArg & 1) == 0) simple_tiles<D, OP, true, true>(a, w, (uint32_t)G, nBytes, nTiles);
          else simple_tiles<D, OP, false, true>(a, w, (uint32_t)G, nBytes, nTiles);
        } else {
          simple_tiles<D, OP, false, true>(a, w, (uint32_t)G, nBytes, nTiles);
        }
      }
      if (stRecv || stSend) {
        // every wave: its stores to the send slots have completed and its loads of the receive slots returned
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
    // postPeer. A workgroup without a tile of the slice posts as well: nobody waits for it on this slice.
    if (lane0) {
      if (stSend) {
        if (owns) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-back has completed before the tail goes out
        }
        for (int j = 0; j < nSend; j++)
          __hip_atomic_store(credit_word(P.sendTail[j], w), ss[j] + sps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (stRecv)
        for (int i = 0; i < nRecv; i++)
          __hip_atomic_store(credit_word(P.recvHead[i], w), rs[i] + sps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (stRecv) {
#pragma unroll
      for (int i = 0; i < MP; i++) rs[i] += sps;
    }
    if (stSend) {
#pragma unroll
      for (int j = 0; j < MP; j++) ss[j] += sps;
    }
  }
}

template <int D>
static const void* simple_group_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&reduce_copy_simple_group_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&reduce_copy_simple_group_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&reduce_copy_simple_group_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&reduce_copy_simple_group_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&reduce_copy_simple_group_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

static const void* simple_group_fn(int dt, int op) {
  switch (dt) {
    case nexrInt8: return simple_group_fn_dt<nexrInt8>(op);
    case nexrUint8: return simple_group_fn_dt<nexrUint8>(op);
    case nexrInt32: return simple_group_fn_dt<nexrInt32>(op);
    case nexrUint32: return simple_group_fn_dt<nexrUint32>(op);
    case nexrInt64: return simple_group_fn_dt<nexrInt64>(op);
    case nexrUint64: return simple_group_fn_dt<nexrUint64>(op);
    case nexrFloat16: return simple_group_fn_dt<nexrFloat16>(op);
    case nexrFloat32: return simple_group_fn_dt<nexrFloat32>(op);
    case nexrFloat64: return simple_group_fn_dt<nexrFloat64>(op);
    case nexrBfloat16: return simple_group_fn_dt<nexrBfloat16>(op);
  }
  return nullptr;
}

hipError_t launch_simple_group(int dt, int op, const SimpleStepsParams* table, int nMembers, int G, hipStream_t s) {
  const void* fn = simple_group_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {&table, &nMembers, &G};
  return hipLaunchKernel(fn, dim3((unsigned)(nMembers * G)), dim3(kBlock), args, 0, s);
}

hipError_t simple_group_blocks_per_cu(int dt, int op, int* blocks) {
  const void* fn = simple_group_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, kBlock, 0);
}

template <int D>
static const void* simple_group_direct_fn_dt(int op) {
  switch (op) {
    case nexrDevSum: return (const void*)&reduce_copy_simple_group_direct_kernel<D, nexrDevSum>;
    case nexrDevProd: return (const void*)&reduce_copy_simple_group_direct_kernel<D, nexrDevProd>;
    case nexrDevMinMax: return (const void*)&reduce_copy_simple_group_direct_kernel<D, nexrDevMinMax>;
    case nexrDevPreMulSum: return (const void*)&reduce_copy_simple_group_direct_kernel<D, nexrDevPreMulSum>;
    case nexrDevSumPostDiv:
      if constexpr (Ty<D>::kIsInt) return (const void*)&reduce_copy_simple_group_direct_kernel<D, nexrDevSumPostDiv>;
      break;
  }
  return nullptr;
}

static const void* simple_group_direct_fn(int dt, int op) {
  switch (dt) {
    case nexrInt8: return simple_group_direct_fn_dt<nexrInt8>(op);
    case nexrUint8: return simple_group_direct_fn_dt<nexrUint8>(op);
    case nexrInt32: return simple_group_direct_fn_dt<nexrInt32>(op);
    case nexrUint32: return simple_group_direct_fn_dt<nexrUint32>(op);
    case nexrInt64: return simple_group_direct_fn_dt<nexrInt64>(op);
    case nexrUint64: return simple_group_direct_fn_dt<nexrUint64>(op);
    case nexrFloat16: return simple_group_direct_fn_dt<nexrFloat16>(op);
    case nexrFloat32: return simple_group_direct_fn_dt<nexrFloat32>(op);
    case nexrFloat64: return simple_group_direct_fn_dt<nexrFloat64>(op);
    case nexrBfloat16: return simple_group_direct_fn_dt<nexrBfloat16>(op);
  }
  return nullptr;
}

hipError_t launch_simple_group_direct(int dt, int op, const SimpleDirectParams* table, int nMembers, int G,
                                      hipStream_t s) {
  const void* fn = simple_group_direct_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  void* args[] = {&table, &nMembers, &G};
  return hipLaunchKernel(fn, dim3((unsigned)(nMembers * G)), dim3(kBlock), args, 0, s);
}

hipError_t simple_group_direct_blocks_per_cu(int dt, int op, int* blocks) {
  const void* fn = simple_group_direct_fn(dt, op);
  if (!fn) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, kBlock, 0);
}

}  // namespace nexr
