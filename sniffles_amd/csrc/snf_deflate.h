// snf_deflate.h - the container layer on the way out: text / pickled blocks -> BGZF members (RFC 1951 deflate, RFC 1952 gzip with the
// BC extra field) -> one contiguous file image.
//
// Reference counterpart: pysam.tabix_index / bgzip behind `--vcf out.vcf.gz` (sniffles:573-584: zlib level 6 on one host thread) and
// gzip.compress in the SNF writer (snf.py:291-298).  Kernels of snf_container.h: nothing else may include this header.
//
//   deflate_member  one workgroup (DZ_WG threads) per member of at most DZ_MAX input bytes, the grid strides over the members.
//                   The member's input lives in LDS.
//                   1 match + parse, in rounds of DZ_WG consecutive positions, a thread per position.  Candidates of a position p:
//                     (a) the nearest earlier position of the SAME round with the same four bytes (a scan back to the round's first
//                         position over LDS), (b) the last position of the EARLIER rounds in p's hash bucket.  The hash table (2^14
//                         dwords, position + 1) is read by the whole round, then - behind a barrier - written with atomicMax: what it
//                         holds never depends on the order of the lanes.  The longer match wins, the nearer one on a tie; a match is
//                         at least DZ_MINLEN long, never reaches past the member's end, never further back than 32768.
//                     Greedy parse of the round: step[t] = match length or 1; the positions reached from the round's first token start
//                     are marked by pointer doubling (jmp[k][t]: the 2^k-th successor of t); a prefix count over the marks gives each
//                     token its index.  Tokens (a dword each) go through HBM (a dword per input byte), the two histograms are LDS atomics.
//                   2 code lengths from the histograms: rank sort by (count, symbol), one lane merges the two queues, depths top down;
//                     a tree deeper than the limit (15 bits - SNF_DEFLATE_MAXBITS lowers it, so that tests reach the limiter -, 7 for the code-length
//                     alphabet) is built again from halved counts.
//                     Canonical codes, the code-length sequence (zero runs as symbols 17 / 18), HLIT / HDIST / HCLEN.
//                   3 the coded size is known before a bit is emitted: if it is not below the stored size, ONE stored block is written
//                     (a member is never longer than its input + 5 + 26 bytes, its slot never overrun).
//                   4 emission: the hash table's LDS is the member image now (zeroed).  DZ_TOK tokens per thread and round, a prefix sum
//                     over their bit lengths gives the positions, a token (at most 48 bits) is OR-ed into up to three dwords.
//                   5 CRC-32: a contiguous chunk per thread, partial CRCs shifted by multiplication with x^(8 * bytes behind) mod P.
//                   6 the image (18-byte header with BSIZE, payload, CRC-32, ISIZE) to the member's slot in 16-byte stores.
//                   No workgroup waits for another; nothing depends on the grid or on the order of lanes.
//   deflate_pack    the members' slots -> the file image at the offsets of a rocPRIM exclusive scan over the member sizes.
#pragma once
#include "snf_lanes.h"

namespace snf {

#define DZ_WG 256                 // threads of a workgroup = positions of a match round
#define DZ_MAX 0xff00             // input bytes of a member at most (htslib's cut)
#define DZ_SLOT 65536             // bytes between the output slots of two members
#define DZ_HBITS 14
#define DZ_TOK 4                  // tokens per thread and emission round
#define DZ_MINLEN 4
#define DZ_MAXLEN 258
#define DZ_MAXDIST 32768
#define DZ_LIMIT 15               // longest literal/length or distance code
#define DZ_CLIMIT 7               // longest code of the code-length alphabet
#define DZ_POLY 0xedb88320u

enum { DZ_OK = 0, DZ_PREDICT = 1 };
enum { DC_NTOK = 0, DC_CARRY, DC_BITPOS, DC_STORED, DC_ERR, DC_BITS, DC_OVER, DC_NSEQ, DC_HLIT, DC_HDIST, DC_HCLEN, DC_CRC, DC_TOTAL, DC_N };

struct DzShared {
  alignas(16) uint8_t in[DZ_MAX + 48];
  alignas(16) uint32_t tab[1 << DZ_HBITS];      // 1: hash bucket -> position + 1 (0: empty); 4 - 6: the member image
  uint32_t lfreq[288], dfreq[32], cfreq[20], wf[288], nw[576];
  uint16_t par[576], sorted[288], lcode[288], dcode[32], ccode[20], clseq[320];
  uint8_t llen[288], dlen[32], clen[20];
  uint16_t step[DZ_WG], jmp[8][DZ_WG + 2];
  uint8_t mark[DZ_WG + 2];
  uint32_t wsum[2][DZ_WG / 64];
  uint32_t crc_tab[256], x2n[32], crc_part[DZ_WG];
  uint32_t ctl[DC_N];
};

struct DeflateView {
  const uint8_t* in; const int64_t* in_off;      // in_off[n + 1]; `in` has 16 bytes of padding behind its end
  uint8_t* slots; uint32_t* size; uint32_t* status; uint32_t* tok; uint32_t limit;      // tok: a dword per input byte, a member's tokens at its in_off; limit: longest literal/length or distance code (DZ_LIMIT; tests: 9 ..)
};

SNF_HD void dz_len_sym(uint32_t len, uint32_t& sym, uint32_t& xb, uint32_t& xv) {
  const uint32_t l = len - 3u;
  if (len == DZ_MAXLEN) { sym = 285; xb = 0; xv = 0; }
  else if (l < 8u) { sym = 257u + l; xb = 0; xv = 0; }
  else { xb = (uint32_t)(31 - __builtin_clz(l)) - 2u; sym = 261u + 4u * xb + ((l >> xb) & 3u); xv = l & ((1u << xb) - 1u); }
}
SNF_HD void dz_dist_sym(uint32_t dist, uint32_t& sym, uint32_t& xb, uint32_t& xv) {
  const uint32_t d = dist - 1u;
  if (d < 4u) { sym = d; xb = 0; xv = 0; }
  else { xb = (uint32_t)(31 - __builtin_clz(d)) - 1u; sym = 2u * xb + 2u + ((d >> xb) & 1u); xv = d & ((1u << xb) - 1u); }
}
SNF_HD uint32_t dz_len_xbits(uint32_t sym) { const uint32_t s = sym - 257u; return (s < 8u || s == 28u) ? 0u : (s - 4u) >> 2; }
SNF_HD uint32_t dz_dist_xbits(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

// a(x) * b(x) mod P in the reflected representation of CRC-32 (bit 31 is x^0)
SNF_HD uint32_t dz_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ DZ_POLY : b >> 1;
  }
  return p;
}
// x^(8 n) mod P from the table of x^(2^k)
SNF_HD uint32_t dz_xpow8(uint32_t n, const uint32_t* x2n) {
  uint32_t p = 0x80000000u;
  for (int k = 3; n; n >>= 1, k++) if (n & 1u) p = dz_mulmod(x2n[k & 31], p);
  return p;
}

// code lengths of freq[0, n) limited to `maxbits` -> len[0, n).  All threads of the workgroup call it.
SNF_D void dz_huff(DzShared& S, const uint32_t* freq, int n, uint32_t maxbits, uint8_t* len, int tid) {
  for (int s = tid; s < n; s += DZ_WG) { S.wf[s] = freq[s]; len[s] = 0; }
  __syncthreads();
  for (;;) {
    for (int s = tid; s < n; s += DZ_WG) {      // rank among the used symbols by (count, symbol)
      const uint32_t f = S.wf[s];
      if (!f) continue;
      int r = 0;
      for (int u = 0; u < n; u++) { const uint32_t g = S.wf[u]; r += (g && (g < f || (g == f && u < s))) ? 1 : 0; }
      S.sorted[r] = (uint16_t)s;
    }
    __syncthreads();
    if (tid == 0) {
      int m = 0;
      for (int u = 0; u < n; u++) m += S.wf[u] != 0;
      uint32_t over = 0;
      if (m == 1) len[S.sorted[0]] = 1;      // a single code of one bit (legal for the distance alphabet)
      else if (m > 1) {
        for (int i = 0; i < m; i++) S.nw[i] = S.wf[S.sorted[i]];
        int i = 0, j = m;
        for (int k = m; k < 2 * m - 1; k++) {      // leaves [0, m) ascending, inner nodes [m, k) ascending: the two smallest
          int pick[2];
          for (int c = 0; c < 2; c++) pick[c] = (i < m && (j >= k || S.nw[i] <= S.nw[j])) ? i++ : j++;
          S.nw[k] = S.nw[pick[0]] + S.nw[pick[1]];
          S.par[pick[0]] = (uint16_t)k; S.par[pick[1]] = (uint16_t)k;
        }
        S.nw[2 * m - 2] = 0;      // depths, top down
        for (int k = 2 * m - 3; k >= 0; k--) {
          const uint32_t d = S.nw[S.par[k]] + 1u;
          S.nw[k] = d;
          if (k < m) { if (d > maxbits) over = 1; len[S.sorted[k]] = (uint8_t)(d < 255u ? d : 255u); }
        }
      }
      S.ctl[DC_OVER] = over;
    }
    __syncthreads();
    if (!S.ctl[DC_OVER]) break;
    for (int s = tid; s < n; s += DZ_WG) { const uint32_t f = S.wf[s]; if (f) S.wf[s] = (f + 1u) >> 1; }      // flatter, and again
    __syncthreads();
  }
  __syncthreads();
}
// canonical codes, bit-reversed for an LSB-first stream (one thread)
SNF_D void dz_codes(const uint8_t* len, int n, uint16_t* code) {
  uint32_t cnt[16], next[16];
  for (int b = 0; b < 16; b++) cnt[b] = 0;
  for (int s = 0; s < n; s++) cnt[len[s] & 15]++;
  cnt[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int b = 1; b < 16; b++) { c = (c + cnt[b - 1]) << 1; next[b] = c; }
  for (int s = 0; s < n; s++) {
    const int l = len[s];
    uint32_t rev = 0;
    if (l) { const uint32_t v = next[l]++; for (int b = 0; b < l; b++) rev |= ((v >> b) & 1u) << (l - 1 - b); }
    code[s] = (uint16_t)rev;
  }
}
// (one thread, nobody else writes the image meanwhile)
SNF_D void dz_put(uint32_t* img, uint32_t& bp, uint32_t val, uint32_t nbits) {
  const uint32_t w = bp >> 5, sh = bp & 31u;
  const uint64_t x = (uint64_t)val << sh;
  img[w] |= (uint32_t)x;
  if (x >> 32) img[w + 1] |= (uint32_t)(x >> 32);
  bp += nbits;
}
SNF_D uint32_t dz_match(const uint8_t* in, uint32_t q, uint32_t p, uint32_t maxl) {
  uint32_t l = 0;
  while (l < maxl && in[q + l] == in[p + l]) l++;
  return l;
}
// exclusive prefix of x over the workgroup, `total` for all; buf: one of the two S.wsum rows (alternate them between calls)
SNF_D uint32_t dz_block_scan(uint32_t x, uint32_t* buf, int tid, uint32_t& total) {
  const int lane = tid & 63, w = tid >> 6;
  const uint32_t incl = x_incl_scan<true>(x, lane);
  if (lane == 63) buf[w] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int k = 0; k < DZ_WG / 64; k++) { const uint32_t s = buf[k]; all += s; if (k < w) before += s; }
  total = all;
  return before + incl - x;
}

__global__ void __launch_bounds__(DZ_WG) deflate_member(const DeflateView v, int64_t n_mem) {
  __shared__ DzShared S;
  const int tid = (int)threadIdx.x;
  uint32_t* const img = S.tab;
  uint8_t* const img8 = (uint8_t*)S.tab;
  {      // tables of the CRC: the byte table, x^(2^k) mod P
    uint32_t c = (uint32_t)tid;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ DZ_POLY : c >> 1;
    S.crc_tab[tid] = c;
    if (tid == 0) { uint32_t p = 0x40000000u; for (int k = 0; k < 32; k++) { S.x2n[k] = p; p = dz_mulmod(p, p); } }
    for (int k = 0; k < 8; k++) S.jmp[k][DZ_WG] = DZ_WG;
  }
  __syncthreads();
  for (int64_t m = (int64_t)blockIdx.x; m < n_mem; m += (int64_t)gridDim.x) {
    const int64_t off = v.in_off[m];
    const uint32_t n = (uint32_t)(v.in_off[m + 1] - off), sh = (uint32_t)off & 15u;
    const uint8_t* const in = S.in + sh;      // LDS copy shifted: LDS and HBM addresses agree modulo 16
    uint32_t* const tokv = v.tok + off;      // (a member has at most as many tokens as bytes)
    // ---- per-member state
    for (uint32_t k = (uint32_t)tid; k < (1u << DZ_HBITS); k += DZ_WG) S.tab[k] = 0;
    for (int s = tid; s < 288; s += DZ_WG) S.lfreq[s] = 0;
    if (tid < 32) S.dfreq[tid] = 0;
    if (tid < 20) S.cfreq[tid] = 0;
    if (tid < DC_N) S.ctl[tid] = 0;
    {
      const uint8_t* src = v.in + (off - sh);
      const uint32_t nvec = (sh + n + 15u) >> 4;
      for (uint32_t k = (uint32_t)tid; k < nvec; k += DZ_WG) *(uint4*)(S.in + 16 * k) = *(const uint4*)(src + 16 * k);
    }
    __syncthreads();
    // ---- CRC-32 of the input: a contiguous chunk per thread, shifted behind the chunks that follow
    {
      const uint32_t cs = (n + DZ_WG - 1) / DZ_WG;
      uint32_t a = (uint32_t)tid * cs, b = a + cs;
      if (a > n) a = n;
      if (b > n) b = n;
      uint32_t c = 0;
      if (b > a) {
        c = 0xffffffffu;
        for (uint32_t i = a; i < b; i++) c = S.crc_tab[(c ^ in[i]) & 0xffu] ^ (c >> 8);
        c ^= 0xffffffffu;
        if (n - b) c = dz_mulmod(dz_xpow8(n - b, S.x2n), c);
      }
      S.crc_part[tid] = c;
    }
    __syncthreads();
    if (tid == 0) { uint32_t c = 0; for (int k = 0; k < DZ_WG; k++) c ^= S.crc_part[k]; S.ctl[DC_CRC] = c; }
    // ---- 1: matches and the greedy parse, a round of DZ_WG positions at a time
    uint32_t ntok = 0, s0 = 0;      // tokens so far; the round's first token start, relative to the round
    const uint32_t rounds = (n + DZ_WG - 1) / DZ_WG;
    for (uint32_t r = 0; r < rounds; r++) {
      const uint32_t base = r * DZ_WG, p = base + (uint32_t)tid;
      const bool can = p + DZ_MINLEN <= n;
      uint32_t word = 0, h = 0, blen = 0, bdist = 0;
      if (can) {
        word = (uint32_t)in[p] | (uint32_t)in[p + 1] << 8 | (uint32_t)in[p + 2] << 16 | (uint32_t)in[p + 3] << 24;
        h = (word * 2654435761u) >> (32 - DZ_HBITS);
      }
      if (can && s0 < DZ_WG) {
        const uint32_t maxl = n - p < DZ_MAXLEN ? n - p : DZ_MAXLEN;      // no compare reads behind the member's end
        const uint32_t e = S.tab[h];
        if (e) {
          const uint32_t q = e - 1u, d = p - q;
          if (d <= DZ_MAXDIST) { const uint32_t l = dz_match(in, q, p, maxl); if (l >= DZ_MINLEN) { blen = l; bdist = d; } }
        }
        uint32_t w = word;
        for (uint32_t d = 1; d <= (uint32_t)tid; d++) {
          w = (w << 8) | in[p - d];
          if (w == word) { const uint32_t l = dz_match(in, p - d, p, maxl); if (l >= blen) { blen = l; bdist = d; } break; }
        }
      }
      const uint32_t st = blen ? blen : 1u;
      S.step[tid] = (uint16_t)st;
      { const uint32_t j = (uint32_t)tid + st; S.jmp[0][tid] = (uint16_t)(j < DZ_WG ? j : DZ_WG); }
      S.mark[tid] = (uint32_t)tid == s0 ? 1 : 0;
      __syncthreads();      // every lane has read the table
      if (can) atomicMax(&S.tab[h], p + 1u);
      if (s0 >= DZ_WG) { s0 -= DZ_WG; __syncthreads(); continue; }      // the round lies inside a match
      for (int k = 1; k < 8; k++) { S.jmp[k][tid] = S.jmp[k - 1][S.jmp[k - 1][tid]]; __syncthreads(); }
      for (int k = 7; k >= 0; k--) {
        const bool mk = S.mark[tid] != 0;
        __syncthreads();
        if (mk) S.mark[S.jmp[k][tid]] = 1;
        __syncthreads();
      }
      const bool is_tok = S.mark[tid] != 0 && p < n;
      uint32_t total;
      const uint32_t idx = dz_block_scan(is_tok ? 1u : 0u, S.wsum[r & 1], tid, total);
      if (is_tok) {
        if (blen) {
          uint32_t ls, ds, xb, xv;
          dz_len_sym(blen, ls, xb, xv); dz_dist_sym(bdist, ds, xb, xv);
          atomicAdd(&S.lfreq[ls], 1u); atomicAdd(&S.dfreq[ds], 1u);
          tokv[ntok + idx] = 0x80000000u | (blen - 3u) << 16 | (bdist - 1u);
        } else {
          atomicAdd(&S.lfreq[in[p]], 1u);
          tokv[ntok + idx] = in[p];
        }
        if ((uint32_t)tid + st >= DZ_WG) S.ctl[DC_CARRY] = (uint32_t)tid + st - DZ_WG;
      }
      ntok += total;
      __syncthreads();
      s0 = S.ctl[DC_CARRY];
    }
    __syncthreads();
    // ---- 2: the codes
    if (tid == 0) S.lfreq[256] = 1;
    __syncthreads();
    dz_huff(S, S.lfreq, 286, v.limit, S.llen, tid);
    dz_huff(S, S.dfreq, 30, v.limit, S.dlen, tid);
    if (tid == 0) {
      dz_codes(S.llen, 286, S.lcode); dz_codes(S.dlen, 30, S.dcode);
      uint32_t hlit = 286, hdist = 30;
      while (hlit > 257 && !S.llen[hlit - 1]) hlit--;
      while (hdist > 1 && !S.dlen[hdist - 1]) hdist--;
      uint32_t nseq = 0;
      for (int part = 0; part < 2; part++) {      // the code lengths as symbols of the code-length alphabet: zero runs as 17 / 18
        const uint8_t* L = part ? S.dlen : S.llen;
        const uint32_t cnt = part ? hdist : hlit;
        for (uint32_t i = 0; i < cnt;) {
          if (L[i]) { S.clseq[nseq++] = L[i]; S.cfreq[L[i]]++; i++; continue; }
          uint32_t run = 1;
          while (i + run < cnt && !L[i + run] && run < 138) run++;
          if (run >= 11) { S.clseq[nseq++] = (uint16_t)(18u | (run - 11u) << 8); S.cfreq[18]++; }
          else if (run >= 3) { S.clseq[nseq++] = (uint16_t)(17u | (run - 3u) << 8); S.cfreq[17]++; }
          else { for (uint32_t k = 0; k < run; k++) S.clseq[nseq++] = 0; S.cfreq[0] += run; }
          i += run;
        }
      }
      int used = 0, which = 0;
      for (int s = 0; s < 19; s++) if (S.cfreq[s]) { used++; which = s; }
      if (used == 1) S.cfreq[which ? 0 : 1] = 1;      // the code-length code must be complete: a second (unused) symbol
      S.ctl[DC_NSEQ] = nseq; S.ctl[DC_HLIT] = hlit; S.ctl[DC_HDIST] = hdist;
    }
    __syncthreads();
    dz_huff(S, S.cfreq, 19, DZ_CLIMIT, S.clen, tid);
    // ---- 3: the coded size; the image's head; stored or coded
    for (uint32_t k = (uint32_t)tid; k < (1u << DZ_HBITS); k += DZ_WG) img[k] = 0;
    __syncthreads();
    if (tid == 0) {
      // order of the code-length code lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
      const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
      const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
      dz_codes(S.clen, 19, S.ccode);
      uint32_t hclen = 19;
      while (hclen > 4) { const int i = (int)hclen - 1; const int o = (int)((i < 12 ? ord_lo >> (5 * i) : ord_hi >> (5 * (i - 12))) & 31u); if (S.clen[o]) break; hclen--; }
      const uint32_t nseq = S.ctl[DC_NSEQ], hlit = S.ctl[DC_HLIT], hdist = S.ctl[DC_HDIST];
      uint32_t bits = 3u + 14u + 3u * hclen;
      for (uint32_t k = 0; k < nseq; k++) { const uint32_t s = S.clseq[k] & 0xffu; bits += S.clen[s] + (s == 17u ? 3u : s == 18u ? 7u : 0u); }
      for (uint32_t s = 0; s < 286; s++) bits += S.lfreq[s] * (S.llen[s] + (s > 256u ? dz_len_xbits(s) : 0u));
      for (uint32_t s = 0; s < 30; s++) bits += S.dfreq[s] * (S.dlen[s] + dz_dist_xbits(s));
      const uint32_t coded = (bits + 7u) >> 3;
      const bool stored = n != 0 && coded >= n + 5u;
      const uint32_t payload = n == 0 ? 2u : stored ? n + 5u : coded;
      const uint32_t total = 18u + payload + 8u;
      img[0] = 0x04088b1fu; img[1] = 0; img[2] = 0x0006ff00u; img[3] = 0x00024342u;
      img[4] = (total - 1u) & 0xffffu;      // BSIZE; the payload begins in the upper half of this dword
      uint32_t bp = 18u * 8u;
      if (n == 0) dz_put(img, bp, 3u, 16);                                 // the empty fixed block of the EOF marker: 03 00
      else if (stored) { dz_put(img, bp, 1u, 8); dz_put(img, bp, n, 16); dz_put(img, bp, n ^ 0xffffu, 16); }
      else {
        dz_put(img, bp, 5u, 3);      // BFINAL, dynamic
        dz_put(img, bp, hlit - 257u, 5); dz_put(img, bp, hdist - 1u, 5); dz_put(img, bp, hclen - 4u, 4);
        for (uint32_t i = 0; i < hclen; i++) dz_put(img, bp, S.clen[(i < 12 ? ord_lo >> (5 * i) : ord_hi >> (5 * (i - 12))) & 31u], 3);
        for (uint32_t k = 0; k < nseq; k++) {
          const uint32_t s = S.clseq[k] & 0xffu;
          dz_put(img, bp, S.ccode[s], S.clen[s]);
          if (s == 17u) dz_put(img, bp, (uint32_t)S.clseq[k] >> 8, 3);
          else if (s == 18u) dz_put(img, bp, (uint32_t)S.clseq[k] >> 8, 7);
        }
      }
      S.ctl[DC_BITPOS] = bp; S.ctl[DC_STORED] = (stored || n == 0) ? 1u : 0u; S.ctl[DC_BITS] = bits; S.ctl[DC_TOTAL] = total;
    }
    __syncthreads();
    const uint32_t total = S.ctl[DC_TOTAL];
    if (S.ctl[DC_STORED]) {
      for (uint32_t i = (uint32_t)tid; i < n; i += DZ_WG) img8[23u + i] = in[i];
    } else {
      // ---- 4: the tokens
      uint32_t bp0 = S.ctl[DC_BITPOS];
      for (uint32_t tb = 0, round = 0; tb < ntok; tb += DZ_WG * DZ_TOK, round++) {
        uint64_t val[DZ_TOK]; uint32_t nb[DZ_TOK], sum = 0;
        for (int j = 0; j < DZ_TOK; j++) {
          const uint32_t i = tb + (uint32_t)tid * DZ_TOK + (uint32_t)j;
          val[j] = 0; nb[j] = 0;
          if (i >= ntok) continue;
          const uint32_t t = tokv[i];
          if (t & 0x80000000u) {
            uint32_t ls, lxb, lxv, ds, dxb, dxv;
            dz_len_sym(((t >> 16) & 0xffu) + 3u, ls, lxb, lxv); dz_dist_sym((t & 0x7fffu) + 1u, ds, dxb, dxv);
            uint64_t x = S.lcode[ls]; uint32_t b = S.llen[ls];
            x |= (uint64_t)lxv << b; b += lxb;
            x |= (uint64_t)S.dcode[ds] << b; b += S.dlen[ds];
            x |= (uint64_t)dxv << b; b += dxb;
            val[j] = x; nb[j] = b;
          } else { val[j] = S.lcode[t]; nb[j] = S.llen[t]; }
          sum += nb[j];
        }
        uint32_t all;
        uint32_t bp = bp0 + dz_block_scan(sum, S.wsum[round & 1], tid, all);
        for (int j = 0; j < DZ_TOK; j++) {
          if (!nb[j]) continue;
          const uint32_t w = bp >> 5, s = bp & 31u;      // up to 48 bits from bit s: three dwords
          const uint64_t lo = val[j] << s;
          const uint32_t hi = s ? (uint32_t)(val[j] >> (64u - s)) : 0u;
          if ((uint32_t)lo) atomicOr(&img[w], (uint32_t)lo);
          if (lo >> 32) atomicOr(&img[w + 1], (uint32_t)(lo >> 32));
          if (hi) atomicOr(&img[w + 2], hi);
          bp += nb[j];
        }
        bp0 += all;
      }
      __syncthreads();
      if (tid == 0) {
        dz_put(img, bp0, S.lcode[256], S.llen[256]);
        if (bp0 - 18u * 8u != S.ctl[DC_BITS]) S.ctl[DC_ERR] = DZ_PREDICT;
      }
    }
    __syncthreads();
    if (tid < 8) {      // CRC-32, ISIZE
      const uint32_t x = tid < 4 ? S.ctl[DC_CRC] : n;
      img8[total - 8u + (uint32_t)tid] = (uint8_t)(x >> (8 * (tid & 3)));
    }
    __syncthreads();
    // ---- 6: the slot
    {
      uint8_t* dst = v.slots + (size_t)m * DZ_SLOT;
      const uint32_t nvec = (total + 15u) >> 4;
      for (uint32_t k = (uint32_t)tid; k < nvec; k += DZ_WG) *(uint4*)(dst + 16 * k) = *(const uint4*)(img8 + 16 * k);
      if (tid == 0) { v.size[m] = total; v.status[m] = S.ctl[DC_ERR]; }
    }
    __syncthreads();      // the LDS is the next member's
  }
}

struct PackView { const uint8_t* slots; const uint32_t* size; const int64_t* off; uint8_t* image; };
__global__ void __launch_bounds__(256) deflate_pack(const PackView v, int64_t n_mem) {
  for (int64_t m = (int64_t)blockIdx.x; m < n_mem; m += (int64_t)gridDim.x) {
    const uint8_t* src = v.slots + (size_t)m * DZ_SLOT;
    uint8_t* dst = v.image + v.off[m];
    const uint32_t sz = v.size[m];
    for (uint32_t i = threadIdx.x; i < sz; i += 256) dst[i] = src[i];
  }
}

}  // namespace snf
