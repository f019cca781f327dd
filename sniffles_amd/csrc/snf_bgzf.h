// snf_bgzf.h - the container layer on the GPU: BGZF members -> inflated BAM stream -> record boundaries -> record heads.
//
// Reference counterpart: pysam / htslib's BGZF reader and record iterator behind `bam.fetch` (leadprov.py:487); the host form of
// the same three steps is sniffles_amd/bam.py (bgzf_inflate, parse_bam).  Kernels of snf_container.h: nothing else may include this header.
//
//   bgzf_inflate_wave   one wave (a 64-thread workgroup) per BGZF member, the grid strides over the members.  RFC 1951 inflate: lane 0
//                       decodes symbols into a batch of up to 64 tokens (a literal or a (length, distance) pair) through a primary
//                       lookup table per alphabet (10 bits literal/length, 9 bits distance; longer codes and the code-length
//                       alphabet by the canonical count / symbol walk); the wave resolves the batch: a prefix sum over the token
//                       lengths gives the output positions, literals are written in parallel, matches are copied in token order
//                       by the whole wave (distance < length: lane i reads start + (i mod distance)).  The member's output window
//                       (at most 64 KB, so a back-reference never leaves it) lives in LDS: back-references read LDS, never the
//                       wave's own global stores; the window goes to HBM at the end in 16-byte stores (the LDS copy is shifted so
//                       that LDS and HBM addresses agree modulo 16).  Compressed bytes are read from HBM in 8-byte words.
//                       Every read of compressed bytes is bounded by the member's payload end, every window write by ISIZE, every
//                       back-reference by the bytes produced so far; a malformed member leaves a status word (BZ_*) and nothing
//                       is read or written out of bounds.  CRC-32 is NOT checked (as in bam.bgzf_inflate).
//   bgzf_inflate_thread the same decoder, a thread per member, window = the output in HBM (SNF_BGZF_THREAD; the second
//                       implementation the tests compare with).
//   bam_chain           record boundaries: one workgroup per member's output range.  A workgroup copies its segment into LDS, takes a
//                       ticket (snf_fused.h chain_ticket: a block takes its ticket when it starts, so its predecessor is running),
//                       waits - bounded - for its predecessor's carry, walks p += 4 + block_size with one lane, publishes its carry.
//                       A chain of dependent LDS reads per record; the carries are a chain of dependent L2 round trips per segment.
//   bam_heads           a thread per record: the first six dwords of the record, then (second launch) its NUL-padded read name.
#pragma once
#include "../../include/sniffles_amd.h"
#include "snf_lanes.h"

namespace snf {

enum { BZ_OK = 0, BZ_BTYPE, BZ_STORED, BZ_LENS, BZ_CODE, BZ_DIST, BZ_SIZE, BZ_INPUT };
static const char* const BZ_TEXT[] = {"ok", "invalid deflate block type", "invalid stored block lengths", "invalid code lengths set",
                                      "invalid literal/length or distance code", "invalid distance too far back", "BGZF block size mismatch",
                                      "deflate payload ends inside a symbol"};
enum { BC_OK = 0, BC_BLOCK_SIZE = 1, BC_TIMEOUT = 2, BC_OVERFLOW = 3 };

#define BZ_LBITS 10
#define BZ_DBITS 9
#define BZ_BATCH 64
#define BZ_WIN 65536

struct BzTables {
  uint16_t lprim[1 << BZ_LBITS], dprim[1 << BZ_DBITS];   // (symbol << 4) | code length; 0: longer than the table or no such code
  uint16_t lcount[16], dcount[16], ccount[16], offs[16];
  uint16_t lsym[288], dsym[32], csym[20];
  uint8_t lens[320];
  uint32_t tok[BZ_BATCH];      // literal: byte << 16; match: distance << 16 | length
  uint32_t tpos[BZ_BATCH];
  uint32_t ctl[8];             // [0] tokens, [1] stored length, [2] stored source, [3] done, [4] error
};

struct BzIn { const uint8_t* p; uint32_t ip, iend; uint64_t bb; int bc; };
typedef uint64_t __attribute__((aligned(1))) bz_u64_any;

// at least 57 valid bits, or every bit the payload still has (the missing ones read as zero and are never counted)
SNF_HD void bz_refill(BzIn& r) {
  if (r.bc > 56) return;
  const uint32_t avail = r.iend - r.ip;
  uint64_t w = 0;
  if (avail >= 8) w = *(const bz_u64_any*)(r.p + r.ip);
  else for (uint32_t k = 0; k < avail; k++) w |= (uint64_t)r.p[r.ip + k] << (8 * k);
  r.bb |= w << r.bc;
  uint32_t n = (uint32_t)(63 - r.bc) >> 3;
  if (n > avail) n = avail;
  r.ip += n; r.bc += 8 * (int)n;
}
SNF_HD uint32_t bz_take(BzIn& r, int n) {      // (the caller checks r.bc < 0: the payload ended inside the field)
  const uint32_t v = (uint32_t)r.bb & ((1u << n) - 1u);
  r.bb >>= n; r.bc -= n;
  return v;
}
// canonical decode, a bit at a time: the code-length alphabet and codes longer than the primary table
SNF_HD int bz_slow(uint32_t bits, const uint16_t* count, const uint16_t* sym, int& len) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; l++) {
    code |= (int)(bits & 1u); bits >>= 1;
    const int c = count[l];
    if (code - c < first) { len = l; return sym[index + (code - first)]; }
    index += c; first += c; first <<= 1; code <<= 1;
  }
  return -1;
}
// kind 0: code lengths, 1: literal/length, 2: distance.  zlib's rules: over-subscribed is an error; incomplete only passes for a
// single code of one bit (or no code at all) outside the code-length alphabet.
SNF_HD int bz_build(BzTables& T, const uint8_t* len, int n, uint16_t* count, uint16_t* sym, uint16_t* prim, int pbits, int kind) {
  for (int l = 0; l < 16; l++) count[l] = 0;
  for (int s = 0; s < n; s++) count[len[s]]++;
  if (prim) for (int e = 0; e < (1 << pbits); e++) prim[e] = 0;
  if (count[0] == n) return BZ_OK;                 // no codes: whatever is decoded with it is an invalid code
  int left = 1, maxl = 0;
  for (int l = 1; l <= 15; l++) {
    left <<= 1; left -= (int)count[l];
    if (left < 0) return BZ_LENS;
    if (count[l]) maxl = l;
  }
  if (left > 0 && (kind == 0 || maxl != 1)) return BZ_LENS;
  T.offs[1] = 0;
  for (int l = 1; l < 15; l++) T.offs[l + 1] = (uint16_t)(T.offs[l] + count[l]);
  for (int s = 0; s < n; s++) if (len[s]) sym[T.offs[len[s]]++] = (uint16_t)s;
  if (prim) {
    uint32_t code = 0; int idx = 0;
    for (int l = 1; l <= 15; l++) {
      for (int k = 0; k < (int)count[l]; k++) {
        const uint32_t s = sym[idx++];
        if (l <= pbits) {
          uint32_t rev = 0;
          for (int b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
          for (uint32_t e = rev; e < (1u << pbits); e += 1u << l) prim[e] = (uint16_t)((s << 4) | (uint32_t)l);
        }
        code++;
      }
      code <<= 1;
    }
  }
  return BZ_OK;
}
// the header of a dynamic block (lane 0)
SNF_HD int bz_dynamic(BzTables& T, BzIn& r) {
  bz_refill(r);
  const int nlen = (int)bz_take(r, 5) + 257, ndist = (int)bz_take(r, 5) + 1, ncode = (int)bz_take(r, 4) + 4;
  if (r.bc < 0) return BZ_INPUT;
  if (nlen > 286 || ndist > 30) return BZ_LENS;
  // order of the code-length code lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
  const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  for (int i = 0; i < 19; i++) T.lens[i] = 0;
  for (int i = 0; i < ncode; i++) {
    bz_refill(r);
    const int o = (int)((i < 12 ? ord_lo >> (5 * i) : ord_hi >> (5 * (i - 12))) & 31u);
    T.lens[o] = (uint8_t)bz_take(r, 3);
    if (r.bc < 0) return BZ_INPUT;
  }
  if (int e = bz_build(T, T.lens, 19, T.ccount, T.csym, nullptr, 0, 0)) return e;
  int idx = 0;
  while (idx < nlen + ndist) {
    bz_refill(r);
    int L = 0;
    const int s = bz_slow((uint32_t)r.bb & 0x7fffu, T.ccount, T.csym, L);
    if (s < 0) return (r.bc < 15 && r.ip >= r.iend) ? BZ_INPUT : BZ_CODE;
    r.bb >>= L; r.bc -= L;
    if (s < 16) T.lens[idx++] = (uint8_t)s;
    else {
      uint8_t prev = 0; int rep;
      if (s == 16) { if (idx == 0) return BZ_LENS; prev = T.lens[idx - 1]; rep = 3 + (int)bz_take(r, 2); }
      else if (s == 17) rep = 3 + (int)bz_take(r, 3);
      else rep = 11 + (int)bz_take(r, 7);
      if (r.bc < 0) return BZ_INPUT;
      if (idx + rep > nlen + ndist) return BZ_LENS;      // (a repeat may run across the literal/length - distance border)
      while (rep--) T.lens[idx++] = prev;
    }
    if (r.bc < 0) return BZ_INPUT;
  }
  if (T.lens[256] == 0) return BZ_LENS;                   // no end-of-block code
  if (int e = bz_build(T, T.lens, nlen, T.lcount, T.lsym, T.lprim, BZ_LBITS, 1)) return e;
  return bz_build(T, T.lens + nlen, ndist, T.dcount, T.dsym, T.dprim, BZ_DBITS, 2);
}
SNF_HD int bz_fixed(BzTables& T) {
  for (int s = 0; s < 288; s++) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  for (int s = 0; s < 32; s++) T.lens[288 + s] = 5;
  if (int e = bz_build(T, T.lens, 288, T.lcount, T.lsym, T.lprim, BZ_LBITS, 1)) return e;
  return bz_build(T, T.lens + 288, 32, T.dcount, T.dsym, T.dprim, BZ_DBITS, 2);
}

// One member: payload `in[0, in_len)` -> `win[0, isize)`.  WAVE: all 64 lanes call it, win is LDS; else one thread, win is the output.
template <bool WAVE>
SNF_HD uint32_t bgzf_member(const uint8_t* in, uint32_t in_len, uint8_t* win, uint32_t isize, BzTables& T) {
  const int lane = x_lane<WAVE>();
  constexpr uint32_t NL = WAVE ? 64 : 1;
  BzIn r{in, 0, in_len, 0, 0};
  uint32_t outpos = 0;
  int mode = 0, final_block = 0;      // lane 0's: 0 = a block header comes next, 1 = inside a Huffman block
  for (;;) {
    if (lane == 0) {
      uint32_t ntok = 0, err = 0, slen = 0, ssrc = 0, done = 0;
      while (ntok < BZ_BATCH) {
        if (mode == 0) {
          if (final_block) { done = 1; break; }
          bz_refill(r);
          const uint32_t h = bz_take(r, 3);
          if (r.bc < 0) { err = BZ_INPUT; break; }
          final_block = (int)(h & 1u);
          const uint32_t bt = h >> 1;
          if (bt == 3) { err = BZ_BTYPE; break; }
          if (bt == 0) {      // stored: the batch so far, then a copy by the wave
            const int drop = r.bc & 7;
            r.bb >>= drop; r.bc -= drop;
            const uint32_t at = r.ip - (uint32_t)(r.bc >> 3);
            if (at + 4 > in_len) { err = BZ_INPUT; break; }
            const uint32_t ln = (uint32_t)in[at] | (uint32_t)in[at + 1] << 8, nl = (uint32_t)in[at + 2] | (uint32_t)in[at + 3] << 8;
            if ((ln ^ 0xffffu) != nl) { err = BZ_STORED; break; }
            if (at + 4 + ln > in_len) { err = BZ_INPUT; break; }
            ssrc = at + 4; slen = ln;
            r.ip = at + 4 + ln; r.bb = 0; r.bc = 0;
            break;
          }
          err = (uint32_t)(bt == 1 ? bz_fixed(T) : bz_dynamic(T, r));
          if (err) break;
          mode = 1;
          continue;
        }
        bz_refill(r);      // 57 bits: a whole length / distance pair (15 + 5 + 15 + 13)
        uint32_t e = T.lprim[(uint32_t)r.bb & ((1u << BZ_LBITS) - 1u)];
        int L = (int)(e & 15u), s = (int)(e >> 4);
        if (!L) { s = bz_slow((uint32_t)r.bb & 0x7fffu, T.lcount, T.lsym, L); if (s < 0) { err = (r.bc < 15 && r.ip >= r.iend) ? BZ_INPUT : BZ_CODE; break; } }
        r.bb >>= L; r.bc -= L;
        if (r.bc < 0) { err = BZ_INPUT; break; }
        if (s < 256) { T.tok[ntok++] = (uint32_t)s << 16; continue; }
        if (s == 256) { mode = 0; continue; }
        s -= 257;
        if (s >= 29) { err = BZ_CODE; break; }
        uint32_t len;
        if (s < 8) len = 3u + (uint32_t)s;
        else if (s == 28) len = 258;
        else { const int x = (s - 4) >> 2; len = ((4u + ((uint32_t)s & 3u)) << x) + 3u + bz_take(r, x); }
        e = T.dprim[(uint32_t)r.bb & ((1u << BZ_DBITS) - 1u)];
        L = (int)(e & 15u); int d = (int)(e >> 4);
        if (!L) { d = bz_slow((uint32_t)r.bb & 0x7fffu, T.dcount, T.dsym, L); if (d < 0) { err = (r.bc < 15 && r.ip >= r.iend) ? BZ_INPUT : BZ_CODE; break; } }
        r.bb >>= L; r.bc -= L;
        if (d >= 30) { err = BZ_CODE; break; }
        uint32_t dist;
        if (d < 4) dist = 1u + (uint32_t)d;
        else { const int x = (d >> 1) - 1; dist = ((2u + ((uint32_t)d & 1u)) << x) + 1u + bz_take(r, x); }
        if (r.bc < 0) { err = BZ_INPUT; break; }
        T.tok[ntok++] = dist << 16 | len;
      }
      T.ctl[0] = ntok; T.ctl[1] = slen; T.ctl[2] = ssrc; T.ctl[3] = done; T.ctl[4] = err;
    }
    x_wave_sync<WAVE>();
    const uint32_t ntok = x_uni<WAVE>(T.ctl[0]), slen = x_uni<WAVE>(T.ctl[1]), ssrc = x_uni<WAVE>(T.ctl[2]), done = x_uni<WAVE>(T.ctl[3]);
    const uint32_t err = x_uni<WAVE>(T.ctl[4]);
    if (err) return err;
    if (ntok) {
      if (WAVE) {
        const uint32_t t = (uint32_t)lane < ntok ? T.tok[lane] : 0u;
        const uint32_t ml = t & 0xffffu;
        const uint32_t l = (uint32_t)lane < ntok ? (ml ? ml : 1u) : 0u;
        const uint32_t incl = x_incl_scan<WAVE>(l, lane);
        const uint32_t total = x_bcast<WAVE>(incl, 63);
        const uint32_t pos = outpos + incl - l;
        if (x_ballot<WAVE>(ml != 0 && (t >> 16) > pos)) return BZ_DIST;      // reaches before the member's first byte
        if (outpos + total > isize) return BZ_SIZE;                          // nothing of the batch is written
        if ((uint32_t)lane < ntok && !ml) win[pos] = (uint8_t)(t >> 16);
        T.tpos[lane] = pos;
        x_wave_sync<WAVE>();
        uint64_t mm = x_ballot<WAVE>(ml != 0);
        while (mm) {
          const int k = x_ctz(mm); mm &= mm - 1;
          const uint32_t tk = T.tok[k], p = T.tpos[k], len = tk & 0xffffu, d = tk >> 16, src = p - d;
          for (uint32_t j = (uint32_t)lane; j < len; j += NL) win[p + j] = win[src + (d >= len ? j : j % d)];
          x_wave_sync<WAVE>();
        }
        outpos += total;
      } else {
        for (uint32_t k = 0; k < ntok; k++) {
          const uint32_t tk = T.tok[k], len = tk & 0xffffu, d = tk >> 16;
          if (!len) { if (outpos + 1 > isize) return BZ_SIZE; win[outpos++] = (uint8_t)d; continue; }
          if (d > outpos) return BZ_DIST;
          if (outpos + len > isize) return BZ_SIZE;
          for (uint32_t j = 0; j < len; j++) win[outpos + j] = win[outpos - d + j];
          outpos += len;
        }
      }
    }
    if (slen) {
      if (outpos + slen > isize) return BZ_SIZE;
      for (uint32_t j = (uint32_t)lane; j < slen; j += NL) win[outpos + j] = in[ssrc + j];
      outpos += slen;
    }
    x_wave_sync<WAVE>();      // (the control words are lane 0's again)
    if (done) break;
  }
  return outpos == isize ? BZ_OK : BZ_SIZE;
}

struct BgzfView {
  const uint8_t* in; const snf_bgzf_member_t* mem; int64_t n_mem; uint8_t* out; uint32_t* status;
};

__global__ void __launch_bounds__(64) bgzf_inflate_wave(const BgzfView v, int64_t n) {
  __shared__ alignas(16) uint8_t win[BZ_WIN + 16];
  __shared__ BzTables T;
  const int lane = threadIdx.x & 63;
  for (int64_t m = (int64_t)blockIdx.x; m < n; m += (int64_t)gridDim.x) {
    const snf_bgzf_member_t mb = v.mem[m];
    const uint32_t isize = mb.isize, sh = (uint32_t)mb.out_off & 15u;      // LDS copy shifted: LDS and HBM addresses agree modulo 16
    uint32_t st = BZ_OK;
    if (isize) st = bgzf_member<true>(v.in + mb.payload_off, mb.payload_len, win + sh, isize, T);
    if (st == BZ_OK && isize) {
      uint8_t* dst = v.out + mb.out_off;
      const uint8_t* w = win + sh;
      uint32_t a = (16u - sh) & 15u;
      if (a > isize) a = isize;
      if ((uint32_t)lane < a) dst[lane] = w[lane];
      const uint32_t nvec = (isize - a) >> 4;
      for (uint32_t k = (uint32_t)lane; k < nvec; k += 64) *(uint4*)(dst + a + 16 * k) = *(const uint4*)(w + a + 16 * k);
      const uint32_t tail = a + 16 * nvec;
      if (tail + (uint32_t)lane < isize) dst[tail + lane] = w[tail + lane];
    }
    if (lane == 0) v.status[m] = st;
    x_wave_sync<true>();      // the window and the tables are the next member's
  }
}

__global__ void __launch_bounds__(64) bgzf_inflate_thread(const BgzfView v, int64_t n) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  BzTables T;
  const snf_bgzf_member_t mb = v.mem[m];
  v.status[m] = mb.isize ? bgzf_member<false>(v.in + mb.payload_off, mb.payload_len, v.out + mb.out_off, mb.isize, T) : (uint32_t)BZ_OK;
}

// ---- record chain ---------------------------------------------------------------------------------------------------
// carry INTO segment t: word 0 = valid << 63 | skip << 26 | partial block_size bytes << 2 | their number; word 1 = valid << 63 | abort << 62 |
// records counted so far.  Zeroed by the host before the launch; the host writes the carry into segment 0 and reads the one out of the last.
struct ChainView {
  const uint8_t* stream; const snf_bgzf_member_t* mem; int64_t n_mem;
  int64_t* rec_off; int64_t rec_cap;
  unsigned long long* carry; uint32_t* ticket; unsigned long long* err;      // err: min over (absolute byte << 4 | BC_*); ~0: none
  int64_t stream_pos, origin, count_in;
  uint32_t spin_max;
};
#define BC_VALID (1ull << 63)
#define BC_ABORT (1ull << 62)

__global__ void __launch_bounds__(64) bam_chain(const ChainView v, int64_t n) {
  __shared__ alignas(16) uint8_t seg[BZ_WIN + 32];
  __shared__ uint32_t tick;
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    const uint32_t t = atomicAdd(v.ticket, 1u);
    if (t + 1 == gridDim.x) *v.ticket = 0;      // every block holds its ticket: clean for the next launch
    tick = t;
  }
  __syncthreads();
  const int64_t t = (int64_t)tick;
  if (t >= n) return;
  const snf_bgzf_member_t mb = v.mem[t];
  const uint32_t L = mb.isize, sh = (uint32_t)mb.out_off & 15u;
  {      // the segment into LDS: aligned 16-byte loads (the stream has 16 bytes of padding behind its end)
    const uint8_t* src = v.stream + (mb.out_off - sh);
    const uint32_t nvec = (sh + L + 15u) >> 4;
    for (uint32_t k = (uint32_t)lane; k < nvec; k += 64) *(uint4*)(seg + 16 * k) = *(const uint4*)(src + 16 * k);
  }
  __syncthreads();
  if (lane != 0) return;
  const uint8_t* S = seg + sh;
  unsigned long long w0 = 0, w1 = 0;
  uint32_t spins = 0;
  for (;;) {      // bounded: a predecessor that never publishes ends in BC_TIMEOUT, not in a hang
    w0 = ld_agent_u64(&v.carry[2 * t]); w1 = ld_agent_u64(&v.carry[2 * t + 1]);
    if ((w0 & BC_VALID) && (w1 & BC_VALID)) break;
    if (++spins > v.spin_max) { atomicMin(v.err, ((unsigned long long)(v.stream_pos + mb.out_off) << 4) | BC_TIMEOUT); w0 = BC_VALID; w1 = BC_VALID | BC_ABORT; break; }
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_s_sleep(8);
#endif
  }
  int64_t skip = (int64_t)((w0 & ~BC_VALID) >> 26);
  uint32_t npart = (uint32_t)(w0 & 3u), part = (uint32_t)(w0 >> 2) & 0xffffffu;
  unsigned long long count = w1 & ~(BC_VALID | BC_ABORT);
  bool abort_chain = (w1 & BC_ABORT) != 0;
  const int64_t abs0 = v.stream_pos + mb.out_off;      // absolute stream position of S[0]
  if (!abort_chain) {
    int64_t p = 0;
    bool have_bs = false; int64_t start = 0; uint32_t bsu = 0;
    if (npart) {      // (skip is 0) the block_size field began in an earlier segment
      while (npart < 4 && p < (int64_t)L) { part |= (uint32_t)S[p] << (8 * npart); npart++; p++; }
      if (npart == 4) { have_bs = true; bsu = part; start = abs0 + p - 4; npart = 0; part = 0; }
    } else if (skip >= (int64_t)L) { skip -= (int64_t)L; p = (int64_t)L; }
    else { p = skip; skip = 0; }
    while (have_bs || p < (int64_t)L) {
      if (!have_bs) {
        if ((int64_t)L - p < 4) { while (p < (int64_t)L) { part |= (uint32_t)S[p] << (8 * npart); npart++; p++; } break; }
        bsu = (uint32_t)S[p] | (uint32_t)S[p + 1] << 8 | (uint32_t)S[p + 2] << 16 | (uint32_t)S[p + 3] << 24;
        start = abs0 + p; p += 4;
      }
      have_bs = false;
      const int32_t bs = (int32_t)bsu;
      if (bs < 32) { atomicMin(v.err, ((unsigned long long)start << 4) | BC_BLOCK_SIZE); abort_chain = true; break; }
      const int64_t slot = (int64_t)count - v.count_in;
      if (slot >= v.rec_cap) { atomicMin(v.err, ((unsigned long long)start << 4) | BC_OVERFLOW); abort_chain = true; break; }
      v.rec_off[slot] = start - v.origin;
      count++;
      p += bs;
      if (p > (int64_t)L) { skip = p - (int64_t)L; p = (int64_t)L; }
    }
  }
  st_agent_u64(&v.carry[2 * (t + 1)], BC_VALID | (unsigned long long)skip << 26 | (unsigned long long)part << 2 | npart);
  st_agent_u64(&v.carry[2 * (t + 1) + 1], BC_VALID | (abort_chain ? BC_ABORT : 0ull) | count);
}

// ---- record heads and names -------------------------------------------------------------------------------------------
struct HeadsView {
  const uint8_t* stream; int64_t stream_len; const int64_t* rec_off; int64_t rel;      // record i starts at stream[rec_off[i] + rel]
  uint32_t* heads; uint8_t* names; uint32_t* max_name; int32_t width, phase;
};
SNF_HD void bam_heads_body(int64_t i, const HeadsView& v) {
  const int64_t o = v.rec_off[i] + v.rel;
  if (v.phase == 0) {
    uint32_t h[6] = {0, 0, 0, 0, 0, 0};
    if (o >= 0 && o + 24 <= v.stream_len) for (int k = 0; k < 6; k++) h[k] = ld_u32(v.stream + o + 4 * k);      // (a head cut by the end of a run stays zero)
    for (int k = 0; k < 6; k++) v.heads[6 * i + k] = h[k];
    if (h[3] & 0xffu) atomicMax(v.max_name, h[3] & 0xffu);
  } else {
    const uint32_t ln = v.heads[6 * i + 3] & 0xffu;
    for (int32_t k = 0; k < v.width; k++) {
      const int64_t q = o + 36 + k;
      v.names[i * v.width + k] = ((uint32_t)k < ln && q >= 0 && q < v.stream_len) ? v.stream[q] : (uint8_t)0;
    }
  }
}
SNF_KERNEL(bam_heads, HeadsView)

}  // namespace snf
