// nexr_flat_pitched.hip — the all-to-all along an inner dimension and the last-dim all-gather in ONE launch
// (nexrFlatAllToAll2D, nexrFlatAllGather2D), for gfx950. Included at the end of nexr_ll.hip behind
// nexr_flat_scatter_v.hip: the LL / LL128 object stays the one code object beside the per-datatype ones, and the
// helpers of the flat files before it (c_tbl / tbl_ld, flat_alltoall_arg, the unaligned access types) are shared by
// inclusion order only.
//
// What it computes. n ranks, R rows, B bytes per block row; a buffer of n * R * B bytes is [n][R][B] (blocks) or
// [R][n][B] (rows). The exchange is out[d][at_out(s, r) + i] = in[s][at_in(d, r) + i]; the gather is
// out[d][r * n * B + s * B + i] = in[s][r * B + i]. Both are bit copies. To the kernel a side is two strides:
//   the source of run (s, r) on rank d is in[s] + d * inBlock + r * inPitch   (the gather: inBlock = 0, inPitch = B)
//   the output is walked in address order; outBlock / outPitch only say which index of a run moves faster there:
//     blocks out (outBlock > outPitch): run g = o / B of out[d] is (s, r) = (g / R, g % R), `inner` = R
//     rows out   (outPitch > outBlock): run g is (r, s) = (g / n, g % n), `inner` = n
// so one kernel serves the four layout pairs and the gather, with no table and no workspace.
//
// The work split. An item is one piece of one OUTPUT buffer in address order: consecutive waves write consecutive
// addresses whatever R and B are. A lane holds two access units of W bytes, half a piece apart; the piece is
// 128 * W bytes. W is the host's choice (template parameter): 16 where B % 16 == 0, 4 where B % 4 == 0, else 1, so
// that no unit straddles two runs. The rank d, the piece, its first run g0 = (q0, m0) and the piece's offset in
// that run are wave-uniform scalar arithmetic. What differs per lane is how far its unit lies behind that run's
// start:
//   B >= piece (wide): a piece meets at most two runs. Both runs' (s, r) and base pointers are scalar arithmetic and
//     scalar loads of the kernel arguments, and a lane selects one by a compare.
//   B <  piece (narrow): the lane's distance is below two pieces, so its run index is a 24-bit division by B and
//     its (s, r) one 32-bit division by `inner`. Rank k's pointer sits in lane k, loaded once per wave from the
//     kernel-argument segment, and the lane fetches in[s] with two ds_bpermute_b32 (the LDS crossbar, no LDS
//     allocated). A block row of 16 bytes still fills all 64 lanes.
// User pointers have no alignment: every access is the unaligned-capable form, offsets are 64-bit, the cache policy
// is plain. The partition is static: no atomics, no polls, no LDS allocation, no scratch, and a capped grid strides
// over the items, so a launch cannot wait on residency.

namespace nexr {

template <int W> struct FlatPitchedUnit;
template <> struct FlatPitchedUnit<16> { typedef u32x4 V; typedef g_cu32x4_a1 Ld; typedef g_u32x4_a1 St; };
template <> struct FlatPitchedUnit<4> { typedef uint32_t V; typedef g_cu32_a1 Ld; typedef g_u32_a1 St; };
template <> struct FlatPitchedUnit<1> { typedef uint8_t V; typedef g_cu8 Ld; typedef g_u8 St; };

template <int W>
__global__ __launch_bounds__(kBlock) void flat_pitched_kernel(FlatPitchedParams P) {
  typedef FlatPitchedUnit<W> U;
  constexpr uint32_t kPiece = 128u * W, kHalf = 64u * W;
  constexpr uint32_t kIn = offsetof(FlatPitchedParams, in), kOut = offsetof(FlatPitchedParams, out);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t B = P.runBytes;
  const uint64_t per = P.piecesPer, nItems = P.nItems, outBytes = P.outBytes;
  const uint64_t nRuns = P.nRuns;
  const uint64_t inBlock = P.inBlock, inPitch = P.inPitch;
  const uint32_t inner = P.inner;
  const bool rowsOut = P.outPitch > P.outBlock;  // the rank moves faster than the row in the output
  const uint64_t nWaves = (uint64_t)gridDim.x * (kBlock / 64);
  const bool wide = B >= (uint64_t)kPiece;  // wave-uniform: a piece meets two runs at the most
  // lane k keeps in[k] (entries beyond n are zero and never selected by a valid unit)
  uint32_t ptrLo = 0, ptrHi = 0;
  if (!wide) {
    const uint64_t mineIn = flat_alltoall_arg(kIn + 8u * lane);
    ptrLo = (uint32_t)mineIn;
    ptrHi = (uint32_t)(mineIn >> 32);
  }
  for (uint64_t it = (uint64_t)blockIdx.x * (kBlock / 64) + wave; it < nItems; it += nWaves) {
    const uint64_t d = it / per, piece = it - d * per;
    const uint64_t pBeg = piece * kPiece;
    const uint64_t g0 = pBeg / B, rem0 = pBeg - g0 * B;  // the piece begins rem0 bytes into run g0
    const uint64_t q0 = g0 / inner;                      // g0 = q0 * inner + m0
    const uint32_t m0 = (uint32_t)(g0 - q0 * inner);
    const uint64_t col = d * inBlock;  // where rank d's block begins in every input
    char* dst = (char*)(uintptr_t)flat_alltoall_arg(kOut + 8u * (uint32_t)d) + pBeg;
    // where the lane's two units are read: the branches differ in the address only, the loads are common
    const char* src[2];
    if (wide) {
      uint64_t q1 = q0;
      uint32_t m1 = m0 + 1u;
      if (m1 == inner) {
        m1 = 0;
        q1 = q0 + 1u;
      }
      if (g0 + 1u >= nRuns) {  // no run behind the last: never selected by a valid unit
        m1 = m0;
        q1 = q0;
      }
      const uint32_t sA = rowsOut ? m0 : (uint32_t)q0, sB = rowsOut ? m1 : (uint32_t)q1;
      const uint64_t rA = rowsOut ? q0 : (uint64_t)m0, rB = rowsOut ? q1 : (uint64_t)m1;
      const uint64_t p0 = flat_alltoall_arg(kIn + 8u * sA) + col + rA * inPitch;
      const uint64_t p1 = flat_alltoall_arg(kIn + 8u * sB) + col + rB * inPitch;
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const uint64_t off = rem0 + lane * (uint32_t)W + (uint32_t)u * kHalf;  // below 2 B: rem0 < B, kPiece <= B
        src[u] = (const char*)(uintptr_t)(off >= B ? p1 + (off - B) : p0 + off);
      }
    } else {
      const uint32_t b32 = (uint32_t)B & (kPiece - 1u), r32 = (uint32_t)rem0 & (kPiece - 1u);
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const uint32_t off = r32 + lane * (uint32_t)W + (uint32_t)u * kHalf;  // below 2 * kPiece
        const uint32_t q = off / b32, within = off - q * b32;
        const uint32_t m = m0 + q;  // m0 < 2^31 and q < 2^12: no wrap
        const uint32_t qq = m / inner, mm = m - qq * inner;
        const uint32_t outer = (uint32_t)q0 + qq;
        // s is below n and r below R where the unit is valid; beyond the output's end nothing is read
        const uint32_t s = rowsOut ? mm : outer, r = rowsOut ? outer : mm;
        const uint32_t lo32 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(s << 2), (int)ptrLo);
        const uint32_t hi32 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(s << 2), (int)ptrHi);
        src[u] = (const char*)(uintptr_t)(((uint64_t)hi32 << 32 | lo32) + col + (uint64_t)r * inPitch + within);
      }
    }
    bool valid[2];
    typename U::V v[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      valid[u] = pBeg + lane * (uint32_t)W + (uint32_t)u * kHalf + (uint32_t)W <= outBytes;
      v[u] = (typename U::V)0u;
      if (valid[u]) v[u] = *(typename U::Ld*)src[u];
    }
#pragma unroll
    for (int u = 0; u < 2; u++)
      if (valid[u]) *(typename U::St*)(dst + lane * (uint32_t)W + (uint32_t)u * kHalf) = v[u];
  }
}

hipError_t launch_flat_pitched(const FlatPitchedParams& p, int width, unsigned grid, hipStream_t s) {
  void* args[] = {const_cast<FlatPitchedParams*>(&p)};
  const void* fn = width == 16  ? (const void*)&flat_pitched_kernel<16>
                   : width == 4 ? (const void*)&flat_pitched_kernel<4>
                                : (const void*)&flat_pitched_kernel<1>;
  return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, s);
}

}  // namespace nexr
