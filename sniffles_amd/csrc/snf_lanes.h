// snf_lanes.h - lane helpers of kernels written once as template <bool WAVE> (WAVE == false: the thread form, one lane, every helper the
// identity), loads at any byte address, the two BAM record readers and the CIGAR masks.  Used by the extraction and the container kernels.
#pragma once
#include "snf_rt.h"
namespace snf {
// ---- lane helpers: WAVE == true only exists in device code ----------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define XDEV 1
#else
#define XDEV 0
#endif

template <bool WAVE> SNF_HD int x_lane() {
#if XDEV
  return WAVE ? (int)(threadIdx.x & 63) : 0;
#else
  return 0;
#endif
}
template <bool WAVE> SNF_HD uint64_t x_ballot(bool p) {
#if XDEV
  if (WAVE) return __ballot(p);
#endif
  return p ? 1ull : 0ull;
}
// inclusive prefix sum over the wave: Hillis-Steele inside each row of 16 lanes through DPP row shifts, then the row
// totals are passed on with row_bcast:15 / row_bcast:31 (gfx9 DPP).  Needs all 64 lanes active.
template <bool WAVE> SNF_HD uint32_t x_incl_scan(uint32_t x, int lane) {
#if XDEV
  if (WAVE) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
  }
#endif
  (void)lane;
  return x;
}
template <bool WAVE> SNF_HD uint32_t x_bcast(uint32_t x, int src) {
#if XDEV
  if (WAVE) return (uint32_t)__shfl((int)x, src, 64);
#endif
  (void)src;
  return x;
}
template <bool WAVE> SNF_HD int64_t x_bcast64(int64_t x, int src) {
#if XDEV
  if (WAVE) return (int64_t)__shfl((long long)x, src, 64);
#endif
  (void)src;
  return x;
}
template <bool WAVE> SNF_HD void x_wave_sync() {
#if XDEV
  if (WAVE) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
#endif
}
// a value every lane holds alike, moved to a scalar register (v_readfirstlane)
template <bool WAVE> SNF_HD uint32_t x_uni(uint32_t x) {
#if XDEV
  if (WAVE) return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
#endif
  return x;
}
template <bool WAVE> SNF_HD uint64_t x_uni64(uint64_t x) { return ((uint64_t)x_uni<WAVE>((uint32_t)(x >> 32)) << 32) | x_uni<WAVE>((uint32_t)x); }
SNF_HD int x_popc(uint64_t m) { return __builtin_popcountll(m); }
SNF_HD int x_ctz(uint64_t m) { return __builtin_ctzll(m); }

SNF_HD uint32_t ld_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
// unaligned little-endian dword: two aligned loads and a funnel shift on the device (the blob is padded by 8 bytes)
SNF_HD uint32_t ld_u32(const uint8_t* p) {
#if XDEV
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  const unsigned sh = (unsigned)(a & 3) * 8;
  const uint32_t lo = q[0];
  if (!sh) return lo;
  return (lo >> sh) | (q[1] << (32 - sh));
#else
  uint32_t v; memcpy(&v, p, 4); return v;
#endif
}
// Loads at any byte address of GLOBAL memory (records are byte-aligned in the blob; the device serves misaligned global accesses
// in hardware, so one instruction fetches what two aligned loads and a shift did).  The blob is padded by 16 bytes.
typedef uint32_t __attribute__((aligned(1))) x_u32_any;
typedef uint4 __attribute__((aligned(1))) x_u128_any;
// 8 bytes at any address of the blob OR of the LDS copy of a record's auxiliary region: the two aligned words around the
// address and a funnel shift (an unaligned 8-byte LDS read is served lane by lane); both have >= 16 bytes of slack behind them
SNF_HD uint64_t x_ld8(const uint8_t* p) {
#if XDEV
  const uintptr_t a = (uintptr_t)p;
  const uint64_t* q = (const uint64_t*)(a & ~(uintptr_t)7);
  const unsigned sh = (unsigned)(a & 7) * 8;
  const uint64_t lo = q[0], hi = q[1];
  return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
#else
  uint64_t w; memcpy(&w, p, 8); return w;
#endif
}
// the first six dwords of a record (block_size, refID, pos, l_read_name | mapq | bin, n_cigar_op | flag, l_seq).  Wave form: one
// dword per lane, read back with v_readlane - the values sit in scalar registers from then on (everything derived from them is
// wave-uniform and costs no vector registers)
template <bool WAVE> SNF_HD void x_header(const uint8_t* R, int lane, uint32_t* hd) {
#if XDEV
  if (WAVE) {
    uint32_t w = 0;
    if (lane < 6) w = *(const x_u32_any*)(R + 4 * lane);
#pragma unroll
    for (int k = 0; k < 6; k++) hd[k] = (uint32_t)__builtin_amdgcn_readlane((int)w, k);
    return;
  }
#endif
  (void)lane;
  for (int k = 0; k < 6; k++) hd[k] = ld_u32(R + 4 * k);
}
// the CIGAR operations [base + lane * OPL, + OPL) of a record; operations past the end read as 0P.  Wave form: one 16-byte
// load per lane (64 lanes: 1 KB of consecutive operations, sixteen 64-byte lines per instruction).
template <bool WAVE> SNF_HD void x_load_ops(const uint8_t* cig, int n_cig, int base, int lane, uint32_t* dst) {
#if XDEV
  if (WAVE) {
    const int k0 = base + lane * 4;
    if (k0 + 4 <= n_cig) {
      const uint4 q = *(const x_u128_any*)(cig + 4 * (int64_t)k0);
      dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) dst[j] = k0 + j < n_cig ? *(const x_u32_any*)(cig + 4 * (int64_t)(k0 + j)) : 6u;
    }
    return;
  }
#endif
  dst[0] = base + lane < n_cig ? ld_u32(cig + 4 * (int64_t)(base + lane)) : 6u;
}
#define X_REFC 0x18Du    // M D N = X consume the reference
#define X_QRYC 0x193u    // M I S = X consume the read (OPTAB add_read, leadprov.py:182-192)
#define X_EVENT 0x016u   // I D S (OPTAB event column)
}  // namespace snf
