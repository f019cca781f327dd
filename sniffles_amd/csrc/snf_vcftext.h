// snf_vcftext.h - the target VCF of force calling as one text buffer in HBM (snf_vcftext_t): its line table, the columns
// `VCF._parse_target` reads off every record line, and the genotyped lines written back - without a Python loop over the lines.
//
// Reference counterpart: `VCF.read_svs_iter` / `rewrite_genotype` (vcf.py:352-481); the host form of the same rules is
// sniffles_amd/vcf.py `_parse_target`, `read_target_table`, `rewrite_genotype_records`, and it stays the judge: a line gets the class
// VT_RECORD only where the kernel is certain that `_parse_target` would not raise and would give the same values.  Everything else
// is VT_HOST and goes through the host parser, line by line.  Kernels of snf_container.h: nothing else may include this header (the lane helpers
// are snf_lanes.h's, the word masks snf_fasta.h's; a bgzip file is inflated by bgzf_inflate_wave straight into the text buffer).
//
// The text has at least 16 readable bytes behind it and starts 16-byte aligned.  Work is cut as in snf_fasta.h:
//
//   vt_lines   <false>: per chunk of VT_CHUNK bytes (a thread one aligned VT_VEC-byte word, VT_WG threads) the number of line starts -
//              byte 0 and every byte behind a '\n' (a last line without '\n' is a line).  rocPRIM scans.  <true>: the same walk; a
//              workgroup scan gives every start its line number.
//   vt_parse   a wave per line over a capped grid that strides.  Pass A walks the line in steps of VT_STEP bytes (a lane one aligned
//              word): the bytes that are not plain, the stripped end, the first eight tabs (ballots and one DPP prefix sum per step; the
//              tab positions go through LDS).  Pass B walks INFO the same way: every lane tests the items that start in its word against
//              the three keys (one 8-byte load per item), the last hit of every key is that of the highest lane of the last step; an
//              item with two '=' is found from two ballots (what the last special byte in front of a lane's word is).  Integers
//              (at most 18 digits) and the type name are then read by every lane alike.  Passes C / D walk a BND's ALT: brackets, ']',
//              the one ':' between the first two brackets.
//   vt_chrom   a thread per line: does the CHROM of this record line differ, byte by byte, from that of the record line in front of it.
//   vt_size / vt_copy   the size of every output row (a span of the text, plus a suffix), rocPRIM scans, a wave per row copies.
// No kernel here waits for another workgroup.  Plain C++ stores only.
#pragma once
#include "../../include/sniffles_amd.h"
#include "snf_lanes.h"
#include "snf_fasta.h"

namespace snf {

#define VT_VEC 16            // bytes a thread takes per step (tests/target_text_cases.py reads these literals)
#define VT_WG 256            // threads of a workgroup of vt_lines
#define VT_STEP 1024         // VT_VEC * 64: bytes a wave of vt_parse takes per step
#define VT_CHUNK 4096        // VT_VEC * VT_WG: bytes a workgroup of vt_lines takes per step
#define VT_CHROM_WG 256      // lines a workgroup of vt_chrom / rows a workgroup of vt_size takes
#define VT_MAX_DIGITS 18     // -?[0-9]{1,18}: what an int64 holds whatever the digits
static_assert(VT_STEP == VT_VEC * 64 && VT_CHUNK == VT_VEC * VT_WG && VT_WG % 64 == 0 && VT_VEC == FA_VEC, "chunk sizes");

typedef uint64_t __attribute__((aligned(1))) vt_u64_any;
typedef uint32_t __attribute__((aligned(1))) vt_u32_any;
typedef uint4 __attribute__((aligned(1))) vt_u128_any;

// bit i: byte i of the word is a printable ASCII byte (0x20 .. 0x7e)
SNF_HD uint32_t vt_mask_print(const uint4& w) {
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int k = 0; k < 4; k++) m |= (uint32_t)((((d[j] >> (8 * k)) & 255u) - 0x20u) <= 0x5eu) << (4 * j + k);
  }
  return m;
}

// ---- vt_lines -------------------------------------------------------------------------------------------------------------
struct VtLinesView {
  const uint8_t* text; int64_t n, n_chunks;
  uint32_t* c_ls;                   // per chunk (n_chunks + 1, the last one zero): line starts
  const int64_t* p_ls;              // their exclusive sum
  int64_t* line_start; int64_t n_lines;
};

template <bool EMIT>
__global__ void __launch_bounds__(VT_WG) vt_lines(const VtLinesView v) {
  __shared__ uint32_t part[VT_WG / 64];
  for (int64_t c = (int64_t)blockIdx.x; c < v.n_chunks; c += (int64_t)gridDim.x) {
    const int64_t p = c * VT_CHUNK + (int64_t)threadIdx.x * VT_VEC;
    uint32_t ls = 0;
    if (p < v.n) {
      const uint4 w = *(const uint4*)(v.text + p);
      const uint32_t ok = fa_valid(p, 0, v.n);
      const uint32_t nl = fa_mask_eq(w, 10u) & ok;
      const uint32_t prev_nl = p == 0 ? 1u : (uint32_t)(v.text[p - 1] == 10);
      ls = ((nl << 1) | prev_nl) & ok;
    }
    uint32_t total = 0;
    const uint32_t ex = fa_block_excl((uint32_t)__builtin_popcount(ls), part, total);
    if constexpr (!EMIT) {
      if (threadIdx.x == 0) v.c_ls[c] = total;
    } else {
      const int64_t k0 = v.p_ls[c] + ex;
      uint32_t m = ls;
      for (int j = 0; m; j++) {
        const int i = __builtin_ctz(m);
        m &= m - 1;
        if (k0 + j < v.n_lines) v.line_start[k0 + j] = p + i;
      }
    }
  }
}

// ---- vt_parse -------------------------------------------------------------------------------------------------------------
struct VtParseView {
  const uint8_t* text; int64_t n;
  const int64_t* line_start;        // n_lines + 1: the last entry is n
  snf_vcftext_line_t* line; int64_t n_lines;
};

// -?[0-9]{1,18} in [a, lim), read by every lane alike.  The number ends at lim, at a ';' (semi_ok) or at the line terminator that
// ends at lim (the last INFO item of an 8-column line carries it, and int() takes it).
SNF_D bool vt_int(const uint8_t* text, int64_t a, int64_t lim, bool semi_ok, int64_t* out) {
  int64_t q = a;
  bool neg = false;
  if (q < lim && text[q] == '-') { neg = true; q++; }
  int64_t v = 0;
  int nd = 0;
  while (q < lim && nd <= VT_MAX_DIGITS) {
    const uint32_t c = (uint32_t)text[q] - (uint32_t)'0';
    if (c > 9u) break;
    v = v * 10 + (int64_t)c; nd++; q++;
  }
  if (nd < 1 || nd > VT_MAX_DIGITS) return false;
  if (q != lim) {
    const uint32_t c = text[q];
    const bool term = (c == 10u && q + 1 == lim) || (c == 13u && q + 2 == lim && text[q + 1] == 10);
    if (!(term || (semi_ok && c == (uint32_t)';'))) return false;
  }
  *out = neg ? -v : v;
  return true;
}

// first byte c in [from, to), else to: wave-uniform, every lane one aligned word per step
SNF_D int64_t vt_find(const uint8_t* text, int64_t from, int64_t to, uint32_t c, int lane) {
  for (int64_t base = from & ~(int64_t)15; base < to; base += VT_STEP) {
    const int64_t p = base + 16 * (int64_t)lane;
    uint32_t m = 0;
    if (p < to) m = fa_mask_eq(*(const uint4*)(text + p), c) & fa_valid(p, from, to);
    const uint64_t hit = x_ballot<true>(m != 0);
    if (hit) {
      const int l = x_ctz(hit);
      return base + 16 * (int64_t)l + __builtin_ctz(x_bcast<true>(m, l));
    }
  }
  return to;
}

// the three INFO keys as the little-endian bytes an 8-byte load at the item's start gives
#define VT_K_SVTYPE 0x455059545653ull        /* "SVTYPE" */
#define VT_K_SVLEN 0x4e454c5653ull           /* "SVLEN" */
#define VT_K_END 0x444e45ull                 /* "END" */
#define VT_SEMI ((uint64_t)';')
#define VT_EQ ((uint64_t)'=')

// one item of INFO that starts at q (q <= ib): which key it opens, or whether it is one of the three names as a bare flag
SNF_D void vt_item(const uint8_t* text, int64_t q, int64_t ib, int64_t& at_type, int64_t& at_len, int64_t& at_end, bool& bare) {
  const uint64_t w = *(const vt_u64_any*)(text + q);
  const int64_t room = ib - q;
  const uint64_t k6 = w & 0xffffffffffffull, k5 = w & 0xffffffffffull, k3 = w & 0xffffffull;
  const uint64_t b6 = (w >> 48) & 255u, b5 = (w >> 40) & 255u, b3 = (w >> 24) & 255u;
  if (k6 == VT_K_SVTYPE && room >= 6) {
    if (room == 6 || b6 == VT_SEMI) bare = true;
    else if (b6 == VT_EQ) at_type = q;
  } else if (k5 == VT_K_SVLEN && room >= 5) {
    if (room == 5 || b5 == VT_SEMI) bare = true;
    else if (b5 == VT_EQ) at_len = q;
  } else if (k3 == VT_K_END && room >= 3) {
    if (room == 3 || b3 == VT_SEMI) bare = true;
    else if (b3 == VT_EQ) at_end = q;
  }
}

// the value every lane gets from the highest lane that has one (at < 0: none), else `keep`
SNF_D int64_t vt_last(int64_t at, int64_t keep) {
  const uint64_t m = x_ballot<true>(at >= 0);
  if (!m) return keep;
  return x_bcast64<true>(at, 63 - __builtin_clzll(m));
}

__global__ void __launch_bounds__(64) vt_parse(const VtParseView v) {
  __shared__ int64_t tp[8];
  const int lane = (int)(threadIdx.x & 63);
  const uint8_t* text = v.text;
  for (int64_t k = (int64_t)blockIdx.x; k < v.n_lines; k += (int64_t)gridDim.x) {
    const int64_t s = v.line_start[k], e1 = v.line_start[k + 1];
    int64_t e = e1;                                       // the content is [s, e): without the final "\n" or "\r\n"
    if (e > s && text[e - 1] == 10) { e--; if (e > s && text[e - 1] == 13) e--; }
    snf_vcftext_line_t o{};
    o.start = s; o.cls = SNF_VT_HOST; o.svtype = -1;
    bool host = e == s || e1 - s >= (1ll << 31);
    // ---- pass A: plain bytes, stripped end, the first eight tabs
    uint32_t n_tab = 0;
    int64_t send = s;
    if (!host) {
      bool bad = false;
      for (int64_t base = s & ~(int64_t)15; base < e; base += VT_STEP) {
        const int64_t p = base + 16 * (int64_t)lane;
        uint32_t tab = 0, nb = 0, nonws = 0;
        if (p < e) {
          const uint4 w = *(const uint4*)(text + p);
          const uint32_t ok = fa_valid(p, s, e);
          tab = fa_mask_eq(w, 9u) & ok;
          nb = ok & ~(vt_mask_print(w) | tab);
          nonws = ok & ~(tab | fa_mask_eq(w, 32u));
        }
        bad |= x_ballot<true>(nb != 0) != 0;
        const uint64_t mw = x_ballot<true>(nonws != 0);
        if (mw) {
          const int hl = 63 - __builtin_clzll(mw);
          send = base + 16 * (int64_t)hl + (32 - __builtin_clz(x_bcast<true>(nonws, hl)));
        }
        if (n_tab < 8) {
          const uint32_t cnt = (uint32_t)__builtin_popcount(tab);
          const uint32_t inc = x_incl_scan<true>(cnt, lane);
          uint32_t j = n_tab + inc - cnt;
          for (uint32_t m = tab; m && j < 8; m &= m - 1, j++) tp[j] = p + __builtin_ctz(m);
          n_tab += x_bcast<true>(inc, 63);
        }
      }
      x_wave_sync<true>();
      const uint32_t c0 = text[s];
      if (bad || c0 == 32u || c0 == 9u) host = true;
      else if (c0 == (uint32_t)'#') { o.cls = SNF_VT_HEADER; o.send = (uint32_t)(send - s); host = true; }      // (done: no columns)
    }
    int64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!host) {
      if (n_tab < 7) host = true;
      else {
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = j < (int)(n_tab < 8 ? n_tab : 8) ? tp[j] : 0;
        if (n_tab == 7 && send != e) host = true;        // an 8-column line ends at its terminator
      }
    }
    x_wave_sync<true>();                                  // tp is the next line's
    if (!host) {
      const bool eight = n_tab == 7;
      const int64_t ia = t[6] + 1, ib = eight ? e1 : t[7];        // INFO as split("\t")[7] of the RAW line gives it
      const int64_t cut8 = eight ? send : (t[7] < send ? t[7] : send);
      int64_t pos = 0, qual = 0;
      if (!vt_int(text, t[0] + 1, t[1], false, &pos)) host = true;
      const int64_t qa = t[4] + 1, qb = t[5];
      if (!host && !(qb - qa == 1 && text[qa] == '.') && !vt_int(text, qa, qb, false, &qual)) host = true;
      // ---- pass B: INFO
      int64_t at_type = -1, at_len = -1, at_end = -1;
      if (!host) {
        bool bare = false, two = false;
        uint32_t carry = 0;                               // an '=' stands between the last ';' (or the start of INFO) and this step
        for (int64_t base = ia & ~(int64_t)15; base < ib; base += VT_STEP) {      // (an empty INFO has no item to look at)
          const int64_t p = base + 16 * (int64_t)lane;
          uint32_t semi = 0, eq = 0;
          int64_t a_t = -1, a_l = -1, a_e = -1;
          bool b = false;
          if (p <= ia && ia < p + 16) vt_item(text, ia, ib, a_t, a_l, a_e, b);      // the first item
          if (p < ib) {
            const uint4 w = *(const uint4*)(text + p);
            const uint32_t ok = fa_valid(p, ia, ib);
            semi = fa_mask_eq(w, (uint32_t)';') & ok;
            eq = fa_mask_eq(w, (uint32_t)'=') & ok;
            for (uint32_t m = semi; m; m &= m - 1) vt_item(text, p + __builtin_ctz(m) + 1, ib, a_t, a_l, a_e, b);
          }
          at_type = vt_last(a_t, at_type); at_len = vt_last(a_l, at_len); at_end = vt_last(a_e, at_end);
          bare |= x_ballot<true>(b) != 0;
          // two '=' in one item
          const uint32_t sp = semi | eq;
          const uint32_t kind = !sp ? 0u : ((eq >> (31 - __builtin_clz(sp))) & 1u) ? 2u : 1u;
          const uint64_t m_any = x_ballot<true>(kind != 0), m_eq = x_ballot<true>(kind == 2u);
          const uint64_t below = m_any & ((1ull << lane) - 1ull);
          uint32_t st = below ? (uint32_t)((m_eq >> (63 - __builtin_clzll(below))) & 1ull) : carry;
          bool dbl = false;
          if (eq) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
              if ((semi >> i) & 1u) st = 0;
              else if ((eq >> i) & 1u) { dbl |= st != 0; st = 1; }
            }
          }
          two |= x_ballot<true>(dbl) != 0;
          if (m_any) carry = (uint32_t)((m_eq >> (63 - __builtin_clzll(m_any))) & 1ull);
        }
        if (bare || two) host = true;
      }
      // ---- defaults from REF / ALT, then what INFO gives
      const int64_t rlen = t[3] - t[2] - 1, aa = t[3] + 1, ab = t[4], alen = ab - aa;
      const int64_t pos0 = pos - 1;
      int32_t svtype = alen > rlen ? 0 : 1;
      int64_t svlen = alen > rlen ? alen : -rlen;
      int64_t end = alen > rlen ? pos0 : pos0 + svlen;
      uint32_t span_a = 0, span_len = 0;
      if (!host && at_type >= 0) {
        const int64_t va = at_type + 7, vb = vt_find(text, va, ib, (uint32_t)';', lane);
        svtype = -1;
        if (vb - va == 3) {
          const uint32_t w = *(const vt_u32_any*)(text + va) & 0xffffffu;
          svtype = w == 0x534e49u ? 0 : w == 0x4c4544u ? 1 : w == 0x505544u ? 2 : w == 0x564e49u ? 3 : (w == 0x444e42u || w == 0x415254u) ? 4 : -1;
        }
        if (svtype < 0) { span_a = (uint32_t)(va - s); span_len = (uint32_t)(vb - va); }
      }
      if (!host && at_len >= 0 && !vt_int(text, at_len + 6, ib, true, &svlen)) host = true;
      if (!host && at_end >= 0 && !vt_int(text, at_end + 4, ib, true, &end)) host = true;
      // ---- BND: the mate from ALT
      int64_t mate_pos = 0;
      uint32_t flags = 0;
      if (!host && svtype == 4) {
        int64_t br[2] = {0, 0};
        int found = 0;
        bool rev = false;
        for (int64_t base = aa & ~(int64_t)15; base < ab; base += VT_STEP) {      // pass C: brackets
          const int64_t p = base + 16 * (int64_t)lane;
          uint32_t close = 0, both = 0;
          if (p < ab) {
            const uint4 w = *(const uint4*)(text + p);
            const uint32_t ok = fa_valid(p, aa, ab);
            close = fa_mask_eq(w, (uint32_t)']') & ok;
            both = close | (fa_mask_eq(w, (uint32_t)'[') & ok);
          }
          rev |= x_ballot<true>(close != 0) != 0;
          uint64_t m = x_ballot<true>(both != 0);
          while (m && found < 2) {
            const int l = x_ctz(m);
            m &= m - 1;
            uint32_t mm = x_bcast<true>(both, l);
            for (; mm && found < 2; mm &= mm - 1) br[found++] = base + 16 * (int64_t)l + __builtin_ctz(mm);
          }
        }
        if (found < 2) host = true;
        else {
          int64_t n_colon = 0, colon = -1;
          const int64_t ca = br[0] + 1, cb = br[1];
          for (int64_t base = ca & ~(int64_t)15; base < cb; base += VT_STEP) {    // pass D: the one ':' between the first two
            const int64_t p = base + 16 * (int64_t)lane;
            uint32_t c = 0;
            if (p < cb) c = fa_mask_eq(*(const uint4*)(text + p), (uint32_t)':') & fa_valid(p, ca, cb);
            const uint64_t m = x_ballot<true>(c != 0);
            if (m) {
              const int l = x_ctz(m);
              if (colon < 0) colon = base + 16 * (int64_t)l + __builtin_ctz(x_bcast<true>(c, l));
            }
            const uint32_t inc = x_incl_scan<true>((uint32_t)__builtin_popcount(c), lane);
            n_colon += x_bcast<true>(inc, 63);
          }
          if (n_colon != 1 || !vt_int(text, colon + 1, cb, false, &mate_pos)) host = true;
          else {
            span_a = (uint32_t)(ca - s); span_len = (uint32_t)(colon - ca);
            flags = (text[aa] == 'N' ? SNF_VT_BND_FIRST : 0u) | (rev ? SNF_VT_BND_REVERSE : 0u);
          }
        }
      }
      if (!host) {
        o.cls = SNF_VT_RECORD; o.svtype = (int8_t)svtype; o.flags = (uint8_t)flags;
        o.pos = pos0; o.svlen = svlen; o.end = end; o.mate_pos = mate_pos;
        o.send = (uint32_t)(send - s); o.cut8 = (uint32_t)(cut8 - s); o.chrom_end = (uint32_t)(t[0] - s);
        o.span_a = span_a; o.span_len = span_len;
      }
    }
    if (lane == 0) v.line[k] = o;
  }
}

// ---- vt_chrom -------------------------------------------------------------------------------------------------------------
// SNF_VT_NEW_CHROM on every record line whose CHROM is not, byte for byte, the CHROM of the record line in front of it
// A thread walks back, line by line, over the lines that are no records (headers, HOST lines) to find that record: behind a block of
// g such lines - tens of thousands of ##contig lines in a cohort VCF - the first record's thread makes g serial reads of one byte
// each, once per block; every other thread finds its neighbour at once.  The cost is bounded by the longest gap, the result exact.
__global__ void __launch_bounds__(VT_CHROM_WG) vt_chrom(const VtParseView v) {
  for (int64_t k = (int64_t)blockIdx.x * VT_CHROM_WG + threadIdx.x; k < v.n_lines; k += (int64_t)gridDim.x * VT_CHROM_WG) {
    snf_vcftext_line_t& me = v.line[k];
    if (me.cls != SNF_VT_RECORD) continue;
    int64_t j = k - 1;
    while (j >= 0 && v.line[j].cls != SNF_VT_RECORD) j--;
    bool differs = j < 0 || v.line[j].chrom_end != me.chrom_end;
    if (!differs) {
      const uint8_t *a = v.text + me.start, *b = v.text + v.line[j].start;
      for (uint32_t i = 0; i < me.chrom_end; i++) if (a[i] != b[i]) { differs = true; break; }
    }
    if (differs) me.flags |= SNF_VT_NEW_CHROM;
  }
}

// ---- vt_size / vt_copy ----------------------------------------------------------------------------------------------------
struct VtCopyView {
  const uint8_t* text;
  const snf_vcftext_line_t* line; int64_t n_lines;      // REWRITE: the resident line table
  const int64_t *row_line; const int32_t* row_suffix;   // REWRITE, per row: its line (-1: the host writes this row), its suffix
  const uint8_t* suffix; const int64_t* suffix_off;     // REWRITE: the suffix table
  const int64_t *row_off, *row_len;                     // gather, per row: a span of the text
  int64_t* size;                                        // per row (n + 1, the last one zero)
  const int64_t* out_off; uint8_t* out; int64_t n;
};

template <bool REWRITE>
__global__ void __launch_bounds__(VT_CHROM_WG) vt_size(const VtCopyView v) {
  for (int64_t r = (int64_t)blockIdx.x * VT_CHROM_WG + threadIdx.x; r < v.n; r += (int64_t)gridDim.x * VT_CHROM_WG) {
    int64_t len = 0;
    if constexpr (REWRITE) {
      const int64_t k = v.row_line[r];
      if (k >= 0) len = (int64_t)v.line[k].cut8 + (v.suffix_off[v.row_suffix[r] + 1] - v.suffix_off[v.row_suffix[r]]);
    } else len = v.row_len[r];
    v.size[r] = len;
  }
}

template <bool REWRITE>
__global__ void __launch_bounds__(64) vt_copy(const VtCopyView v) {
  const int64_t lane = (int64_t)(threadIdx.x & 63);
  for (int64_t r = (int64_t)blockIdx.x; r < v.n; r += (int64_t)gridDim.x) {
    int64_t src = 0, len = 0;
    if constexpr (REWRITE) {
      const int64_t k = v.row_line[r];
      if (k < 0) continue;
      src = v.line[k].start; len = v.line[k].cut8;
    } else { src = v.row_off[r]; len = v.row_len[r]; }
    uint8_t* dst = v.out + v.out_off[r];
    const int64_t whole = len & ~(int64_t)15;
    for (int64_t i = 16 * lane; i < whole; i += VT_STEP) *(vt_u128_any*)(dst + i) = *(const vt_u128_any*)(v.text + src + i);
    if (whole + lane < len) dst[whole + lane] = v.text[src + whole + lane];
    if constexpr (REWRITE) {
      const int64_t sa = v.suffix_off[v.row_suffix[r]], sl = v.suffix_off[v.row_suffix[r] + 1] - sa;
      for (int64_t i = lane; i < sl; i += 64) dst[len + i] = v.suffix[sa + i];
    }
  }
}

}  // namespace snf
