// nexr_flat_alltoall.hip — the personalised exchange in ONE launch (nexrFlatAllToAll), for gfx950. Included at the
// end of nexr_ll.hip behind nexr_flat_group.hip: the LL / LL128 object stays the one code object beside the
// per-datatype ones, and the helpers of the flat files before it (kFlatPiece, c_tbl / tbl_ld, the unaligned pack
// types) are shared by inclusion order only.
//
// What it computes. For n ranks and B bytes per pair, out[d][s * B + i] = in[s][d * B + i] for all s, d < n and
// i < B: a bit copy, no datatype, no semantics mode. Block (s -> d) is a pure function of n, B and the 2n base
// pointers, so there is no table, no workspace and no fill launch at any n up to NEXR_SYM_MAX_RANKS: the
// arguments are the two pointer arrays and three numbers.
//
// The pack instance (B % 16 == 0), flat_alltoall_kernel<false>. An item is one kFlatPiece piece of one OUTPUT row
// out[d], n * B bytes long: consecutive waves write consecutive addresses of one row, whatever B is, and a lane
// holds two 16-byte packs 1024 bytes apart as in nexr_flat.hip. The row d, the piece, the first source rank s0 of
// the piece and the piece's offset inside s0's block are wave-uniform scalar arithmetic (two scalar divisions per
// item). No pack straddles two blocks, so a lane at row offset o reads in[o / B] + d * B + o % B; what differs per
// lane is only how far its pack lies behind the piece's first block:
//   B >= kFlatPiece: a piece meets at most two blocks. in[s0] and in[s0 + 1] are scalar loads of the kernel
//     arguments and a lane selects one by a compare: no division and no cross-lane traffic per lane.
//   B <  kFlatPiece: a piece meets up to 128 blocks (B = 16), and the two packs of one lane may come from
//     different ranks. The lane's distance from the block's start is below 4096, so its quotient by B is a
//     24-bit division; rank r's pointer sits in lane r, loaded once per wave from the kernel-argument segment
//     (n <= 64 is the wave width), and the lane fetches in[s] with two ds_bpermute_b32 (the LDS crossbar, no LDS
//     allocated). A 256-byte block fills all 64 lanes this way.
// The byte instance (B % 16 != 0), flat_alltoall_kernel<true>: an item is a piece of ONE block (d, s, piece), all
// wave-uniform, copied as flat_group_copy_kernel copies a record: packs, then the block's last B & 15 bytes one per
// lane. Correct for any B >= 1; rows are then written block by block.
//
// User pointers have no alignment: every pack access is the unaligned-capable form, offsets are 64-bit, the cache
// policy is plain. The partition is static: no atomics, no polls, no LDS allocation, no scratch, and a capped grid
// strides over the items, so a launch cannot wait on residency.

namespace nexr {

// in[r] / out[r] of the kernel arguments as a constant-address-space load: scalar where r is wave-uniform, one
// global load per lane where it is not (indexing the by-value struct per lane would put it in scratch).
__device__ __forceinline__ uint64_t flat_alltoall_arg(uint32_t byteAt) {
  return tbl_ld<uint64_t>((c_tbl*)__builtin_amdgcn_kernarg_segment_ptr() + byteAt);
}

template <bool Bytes>
__global__ __launch_bounds__(kBlock) void flat_alltoall_kernel(FlatAllToAllParams P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = (uint32_t)P.nRanks;
  const uint64_t B = P.blockBytes;
  const uint64_t per = P.piecesPer;  // pieces of a row (packs) or of a block (bytes)
  const uint64_t nItems = P.nItems;
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  constexpr uint32_t kIn = offsetof(FlatAllToAllParams, in), kOut = offsetof(FlatAllToAllParams, out);

  if constexpr (Bytes) {
    for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
      const uint64_t blk = it / per, piece = it - blk * per;
      const uint32_t d = (uint32_t)(blk / n), s = (uint32_t)(blk - (uint64_t)d * n);
      const char* src = (const char*)(uintptr_t)flat_alltoall_arg(kIn + 8u * s) + (uint64_t)d * B;
      char* dst = (char*)(uintptr_t)flat_alltoall_arg(kOut + 8u * d) + (uint64_t)s * B;
      const uint64_t pBeg = piece * kFlatPiece;
      const uint64_t pEnd = pBeg + kFlatPiece < B ? pBeg + kFlatPiece : B;
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
      const uint32_t tail = (uint32_t)(B & 15u);
      const bool last = pEnd == B && lane < tail;
      const uint64_t to = (B & ~(uint64_t)15) + lane;
      uint8_t b = 0;
      if (last) b = *(g_cu8*)(src + to);
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (valid[u]) *(g_u32x4_a1*)(dst + mine + u * (kFlatPiece / 2)) = v[u];
      if (last) *(g_u8*)(dst + to) = b;
    }
  } else {
    const uint64_t rowBytes = (uint64_t)n * B;
    const bool wide = B >= (uint64_t)kFlatPiece;  // wave-uniform: a piece meets two blocks at the most
    // lane r keeps in[r] (entries beyond n are zero and never selected)
    uint32_t ptrLo = 0, ptrHi = 0;
    if (!wide) {
      const uint64_t mineIn = flat_alltoall_arg(kIn + 8u * lane);
      ptrLo = (uint32_t)mineIn;
      ptrHi = (uint32_t)(mineIn >> 32);
    }
    for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
      const uint64_t d = it / per, piece = it - d * per;
      const uint64_t pBeg = piece * kFlatPiece;
      const uint64_t s0 = pBeg / B, rem0 = pBeg - s0 * B;  // the piece begins rem0 bytes into block (s0 -> d)
      const uint64_t col = d * B;                          // where rank d's blocks begin in every input
      char* dst = (char*)(uintptr_t)flat_alltoall_arg(kOut + 8u * (uint32_t)d) + pBeg;
      // where the lane's two packs are read: the branches differ in the address only, the loads are common
      const char* src[2];
      if (wide) {
        const uint32_t s1 = (uint32_t)s0 + 1u < n ? (uint32_t)s0 + 1u : (uint32_t)s0;
        const uint64_t p0 = flat_alltoall_arg(kIn + 8u * (uint32_t)s0) + col;
        const uint64_t p1 = flat_alltoall_arg(kIn + 8u * s1) + col;
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const uint64_t off = rem0 + lane * 16u + (uint32_t)u * (kFlatPiece / 2);  // below 2 B: rem0 < B, kFlatPiece <= B
          src[u] = (const char*)(uintptr_t)(off >= B ? p1 + (off - B) : p0 + off);
        }
      } else {
        const uint32_t b32 = (uint32_t)B & (kFlatPiece - 1u), r32 = (uint32_t)rem0 & (kFlatPiece - 1u);
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const uint32_t off = r32 + lane * 16u + (uint32_t)u * (kFlatPiece / 2);  // below 2 * kFlatPiece
          const uint32_t q = off / b32, within = off - q * b32;
          const uint32_t s = (uint32_t)s0 + q;  // below n where the pack is valid; beyond it nothing is read
          const uint32_t lo32 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(s << 2), (int)ptrLo);
          const uint32_t hi32 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(s << 2), (int)ptrHi);
          src[u] = (const char*)(uintptr_t)(((uint64_t)hi32 << 32 | lo32) + col + within);
        }
      }
      bool valid[2];
      u32x4 v[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        valid[u] = pBeg + lane * 16u + (uint32_t)u * (kFlatPiece / 2) + 16u <= rowBytes;
        v[u] = (u32x4)0u;
        if (valid[u]) v[u] = *(g_cu32x4_a1*)src[u];
      }
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (valid[u]) *(g_u32x4_a1*)(dst + lane * 16u + u * (kFlatPiece / 2)) = v[u];
    }
  }
}

hipError_t launch_flat_alltoall(const FlatAllToAllParams& p, bool bytes, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<FlatAllToAllParams*>(&p)};
  const void* fn = bytes ? (const void*)&flat_alltoall_kernel<true> : (const void*)&flat_alltoall_kernel<false>;
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

}  // namespace nexr
