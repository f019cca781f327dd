// snf_fasta.h - the reference FASTA as one text buffer in HBM (snf_fasta_t): its `.fai` table, the runs of 'N' of a base range and
// batched base fetches, without the text ever returning to the host.
//
// Reference counterpart: pysam.FastaFile behind `_mask_N_coverage` (leadprov.py:420-443) and the VCF writer's REF / ALT resolution
// (vcf.py:108-120, 302-342); the host form of the same rules is sniffles_amd/fasta.py FastaFile (`_scan_bytes`, `fetch`).  Kernels of
// snf_container.h: nothing else may include this header (the lane helpers are snf_lanes.h's; a bgzip reference is inflated by
// snf_bgzf.h's bgzf_inflate_wave straight into the text buffer).
//
// The text has at least 16 readable bytes behind it and starts 16-byte aligned.  Text offsets are 64-bit, base coordinates 32-bit.
// Work is cut alike in fa_index and fa_nruns: a thread takes one aligned FA_VEC-byte word, a wave FA_WAVE_BYTES, a workgroup of FA_WG
// threads one chunk of FA_CHUNK bytes per step, and a capped grid (SNF_FASTA_GRID) strides over the chunks.
//
//   fa_index   <false>: per chunk the number of '\n', of line-end '\r' (a '\r' in front of a '\n' or of the end of the text - what
//              `_scan_bytes` takes off a line's bases) and of header lines (a '>' at byte 0 or behind a '\n').  rocPRIM scans the three
//              columns.  <true>: the same walk; a workgroup scan (LDS: the four wave totals) gives every header its record number and
//              the counts of '\n' / line-end '\r' in front of it.  fa_lines, a wave per record, then finds the end of the header line
//              and of the first sequence line (every lane a 16-byte word per step).  The host subtracts neighbours: the counts of a
//              record's span.
//   fa_nruns   the runs of the byte 'N' (78, upper case only) of the text range [b0, b1) that holds the bases [lo, hi) of a contig.
//              '\n' and '\r' are transparent: a run opens at an 'N' whose previous BASE byte is not 'N' and closes behind an 'N' whose
//              next base byte is not 'N'; a word whose first (last) base is an 'N' looks back (ahead) over the line end, bounded by
//              the range.  <false> counts opens, closes and line-end bytes per chunk; rocPRIM scans; <true> writes the k-th open and
//              the k-th close as run k.  A base coordinate is lo + (text bytes since b0) - (line-end bytes since b0): counted, never
//              divided, and exact whatever the line width.  The line-end total tells the host whether [b0, b1) held hi - lo bases.
//   fa_gather  a wave per query over a striding grid: the lanes take 64 bases per step.  A lane divides once per query (32 bits:
//              its first base -> line, column) and then advances by 64 % line_bases columns and 64 / line_bases lines per step.  The
//              bases go to the pool at off[q], the wave counts its 'N' bytes by ballot.
// No kernel here waits for another workgroup.  Plain C++ stores only.
#pragma once
#include "snf_lanes.h"
#include "snf_bgzf.h"

namespace snf {

#define FA_VEC 16            // bytes a thread takes per step (tests/fasta_cases.py reads these four literals)
#define FA_WG 256            // threads of a workgroup of fa_index / fa_nruns
#define FA_WAVE_BYTES 1024   // FA_VEC * 64
#define FA_CHUNK 4096        // FA_VEC * FA_WG: bytes a workgroup takes per step
#define FA_GATHER_STEP 64    // bases a wave of fa_gather takes per step
static_assert(FA_WAVE_BYTES == FA_VEC * 64 && FA_CHUNK == FA_VEC * FA_WG && FA_WG % 64 == 0, "chunk sizes");

struct FaRec { int64_t pos, nl_before, cr_before, hdr_end, line_end, line_cr; };      // one header line (48 bytes)

// bit i: byte i of the word equals c
SNF_HD uint32_t fa_mask_eq(const uint4& w, uint32_t c) {
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int k = 0; k < 4; k++) m |= (uint32_t)(((d[j] >> (8 * k)) & 255u) == c) << (4 * j + k);
  }
  return m;
}
// bit i: a <= p + i < b
SNF_HD uint32_t fa_valid(int64_t p, int64_t a, int64_t b) {
  const int64_t lo = a - p, hi = b - p;
  const int l = lo < 0 ? 0 : lo > 16 ? 16 : (int)lo, h = hi < 0 ? 0 : hi > 16 ? 16 : (int)hi;
  return h > l ? ((1u << h) - 1u) & ~((1u << l) - 1u) : 0u;
}
// exclusive prefix of x over the FA_WG threads of the workgroup, and the total (LDS: one word per wave).  Every thread calls it.
SNF_D uint32_t fa_block_excl(uint32_t x, uint32_t* part, uint32_t& total) {
  const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
  const uint32_t inc = x_incl_scan<true>(x, lane);
  if (lane == 63) part[w] = inc;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < FA_WG / 64; k++) { const uint32_t t = part[k]; if (k < w) base += t; sum += t; }
  __syncthreads();      // the partials are the next scan's
  total = sum;
  return base + inc - x;
}

// ---- fa_index -------------------------------------------------------------------------------------------------------------
struct FaIndexView {
  const uint8_t* text; int64_t n, n_chunks;
  uint32_t *c_nl, *c_cr, *c_hdr;                      // per chunk (n_chunks + 1, the last one zero)
  const int64_t *p_nl, *p_cr, *p_hdr;                 // their exclusive sums
  FaRec* rec; int64_t n_rec;
};

template <bool EMIT>
__global__ void __launch_bounds__(FA_WG) fa_index(const FaIndexView v) {
  __shared__ uint32_t part[FA_WG / 64];
  for (int64_t c = (int64_t)blockIdx.x; c < v.n_chunks; c += (int64_t)gridDim.x) {
    const int64_t p = c * FA_CHUNK + (int64_t)threadIdx.x * FA_VEC;
    uint32_t nl = 0, cr = 0, hd = 0;
    if (p < v.n) {
      const uint4 w = *(const uint4*)(v.text + p);
      const uint32_t ok = fa_valid(p, 0, v.n);
      nl = fa_mask_eq(w, 10u) & ok;
      uint32_t follow = nl >> 1;                      // bit i: byte i + 1 is a '\n' - or the end of the text
      if (v.n - p <= 16) follow |= 1u << (int)(v.n - p - 1);
      else follow |= (uint32_t)(v.text[p + 16] == 10) << 15;
      cr = fa_mask_eq(w, 13u) & ok & follow;
      const uint32_t prev_nl = p == 0 ? 1u : (uint32_t)(v.text[p - 1] == 10);
      hd = fa_mask_eq(w, (uint32_t)'>') & ok & ((nl << 1) | prev_nl) & 0xffffu;
    }
    uint32_t t_cnt = 0, t_hd = 0;
    const uint32_t ex_cnt = fa_block_excl((uint32_t)__builtin_popcount(nl) | (uint32_t)__builtin_popcount(cr) << 16, part, t_cnt);
    const uint32_t ex_hd = fa_block_excl((uint32_t)__builtin_popcount(hd), part, t_hd);
    if constexpr (!EMIT) {
      if (threadIdx.x == 0) { v.c_nl[c] = t_cnt & 0xffffu; v.c_cr[c] = t_cnt >> 16; v.c_hdr[c] = t_hd; }
    } else {
      const int64_t k0 = v.p_hdr[c] + ex_hd, nl0 = v.p_nl[c] + (ex_cnt & 0xffffu), cr0 = v.p_cr[c] + (ex_cnt >> 16);
      uint32_t m = hd;
      for (int j = 0; m; j++) {
        const int i = __builtin_ctz(m);
        m &= m - 1;
        const uint32_t below = (1u << i) - 1u;
        if (k0 + j < v.n_rec) {
          FaRec& r = v.rec[k0 + j];
          r.pos = p + i; r.nl_before = nl0 + __builtin_popcount(nl & below); r.cr_before = cr0 + __builtin_popcount(cr & below);
        }
      }
    }
  }
}

// first '\n' in [from, n), else n: wave-uniform, every lane one aligned word per step
SNF_D int64_t fa_find_nl(const uint8_t* text, int64_t n, int64_t from, int lane) {
  for (int64_t base = from & ~(int64_t)15; base < n; base += FA_WAVE_BYTES) {
    const int64_t p = base + 16 * (int64_t)lane;
    uint32_t m = 0;
    if (p < n) m = fa_mask_eq(*(const uint4*)(text + p), 10u) & fa_valid(p, from, n);
    const uint64_t hit = x_ballot<true>(m != 0);
    if (hit) {
      const int l = x_ctz(hit);
      return base + 16 * (int64_t)l + __builtin_ctz(x_bcast<true>(m, l));
    }
  }
  return n;
}

// a wave per header line: the end of the header line, the end of the first sequence line and whether that line ends in '\r'
__global__ void __launch_bounds__(64) fa_lines(const FaIndexView v) {
  const int lane = (int)(threadIdx.x & 63);
  for (int64_t k = (int64_t)blockIdx.x; k < v.n_rec; k += (int64_t)gridDim.x) {
    const int64_t h = v.rec[k].pos;
    const int64_t he = fa_find_nl(v.text, v.n, h, lane);
    const int64_t ls = he + 1;
    const int64_t le = ls < v.n ? fa_find_nl(v.text, v.n, ls, lane) : v.n;
    if (lane == 0) {
      v.rec[k].hdr_end = he; v.rec[k].line_end = le;
      v.rec[k].line_cr = (ls < v.n && le > ls && v.text[le - 1] == 13) ? 1 : 0;
    }
  }
}

// ---- fa_nruns -------------------------------------------------------------------------------------------------------------
struct FaRunsView {
  const uint8_t* text; int64_t b0, b1, a0, n_chunks; int32_t lo;      // the text range, its first word, the first base
  unsigned long long* c_se; uint32_t* c_le;          // per chunk (n_chunks + 1): opens | closes << 32, line-end bytes
  const unsigned long long* p_se; const int64_t* p_le;
  int32_t *start, *end; int64_t n_runs;
};
SNF_HD bool fa_is_le(uint32_t b) { return b == 10u || b == 13u; }

template <bool EMIT>
__global__ void __launch_bounds__(FA_WG) fa_nruns(const FaRunsView v) {
  __shared__ uint32_t part[FA_WG / 64];
  for (int64_t c = (int64_t)blockIdx.x; c < v.n_chunks; c += (int64_t)gridDim.x) {
    const int64_t p = v.a0 + c * FA_CHUNK + (int64_t)threadIdx.x * FA_VEC;
    uint32_t nm = 0, le = 0, base = 0, opens = 0, closes = 0;      // masks over the word's bytes
    if (p < v.b1) {
      const uint4 w = *(const uint4*)(v.text + p);
      const uint32_t ok = fa_valid(p, v.b0, v.b1);
      le = (fa_mask_eq(w, 10u) | fa_mask_eq(w, 13u)) & ok;
      base = ok & ~le;
      nm = fa_mask_eq(w, 78u) & base;
      if (nm) {
        bool prev_n = false;
        if (nm & base & (0u - base)) {      // the word's first base is an 'N': what is the base in front of the word?
          int64_t q = p - 1;
          while (q >= v.b0 && fa_is_le(v.text[q])) q--;
          prev_n = q >= v.b0 && v.text[q] == 78;
        }
        int pending = -1;                   // the last base so far, if it is an 'N' whose successor is not known yet
#pragma unroll
        for (int i = 0; i < 16; i++) {
          if (!((base >> i) & 1u)) continue;
          const bool is_n = (nm >> i) & 1u;
          if (is_n && !prev_n) opens |= 1u << i;
          if (!is_n && pending >= 0) closes |= 1u << pending;
          pending = is_n ? i : -1;
          prev_n = is_n;
        }
        if (pending >= 0) {                 // the word's last base is an 'N': what is the base behind the word?
          int64_t q = p + 16;
          while (q < v.b1 && fa_is_le(v.text[q])) q++;
          if (!(q < v.b1 && v.text[q] == 78)) closes |= 1u << pending;
        }
      }
    }
    uint32_t t_se = 0, t_le = 0;
    const uint32_t ex_se = fa_block_excl((uint32_t)__builtin_popcount(opens) | (uint32_t)__builtin_popcount(closes) << 16, part, t_se);
    const uint32_t ex_le = fa_block_excl((uint32_t)__builtin_popcount(le), part, t_le);
    if constexpr (!EMIT) {
      if (threadIdx.x == 0) { v.c_se[c] = (unsigned long long)(t_se & 0xffffu) | (unsigned long long)(t_se >> 16) << 32; v.c_le[c] = t_le; }
    } else {
      const unsigned long long se0 = v.p_se[c];
      const int64_t s0 = (int64_t)(se0 & 0xffffffffull) + (ex_se & 0xffffu), e0 = (int64_t)(se0 >> 32) + (ex_se >> 16);
      const int64_t coord0 = (int64_t)v.lo + (p - v.b0) - (v.p_le[c] + ex_le);      // base coordinate of byte 0 of the word, were it a base
      uint32_t m = opens;
      for (int j = 0; m; j++) {
        const int i = __builtin_ctz(m);
        m &= m - 1;
        if (s0 + j < v.n_runs) v.start[s0 + j] = (int32_t)(coord0 + i - __builtin_popcount(le & ((1u << i) - 1u)));
      }
      m = closes;
      for (int j = 0; m; j++) {
        const int i = __builtin_ctz(m);
        m &= m - 1;
        if (e0 + j < v.n_runs) v.end[e0 + j] = (int32_t)(coord0 + i - __builtin_popcount(le & ((1u << i) - 1u)) + 1);
      }
    }
  }
}

// ---- fa_gather ------------------------------------------------------------------------------------------------------------
struct FaGatherView {
  const uint8_t* text; int64_t offset; uint32_t lb, lw;      // the contig's first base, bases and bytes of a line
  const int32_t *start, *len; const int64_t* off;            // per query: first base, clipped length, place in the pool
  uint8_t* pool; int32_t* n_count;
};
__global__ void __launch_bounds__(64) fa_gather(const FaGatherView v, int64_t n) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t adv_line = FA_GATHER_STEP / v.lb, adv_col = FA_GATHER_STEP % v.lb;
  for (int64_t q = (int64_t)blockIdx.x; q < n; q += (int64_t)gridDim.x) {
    const uint32_t s = (uint32_t)v.start[q], L = (uint32_t)v.len[q];
    const int64_t o = v.off[q];
    uint32_t cnt = 0;
    if (L) {
      uint32_t line = (s + lane) / v.lb, col = (s + lane) % v.lb;
      for (uint32_t done = 0; done < L; done += FA_GATHER_STEP) {
        const uint32_t j = done + lane;
        uint32_t b = 0;
        if (j < L) {
          b = v.text[v.offset + (int64_t)line * v.lw + col];
          v.pool[o + j] = (uint8_t)b;
        }
        cnt += (uint32_t)x_popc(x_ballot<true>(b == 78u));
        col += adv_col; line += adv_line;
        if (col >= v.lb) { col -= v.lb; line++; }
      }
    }
    if (lane == 0) v.n_count[q] = (int32_t)cnt;
  }
}

}  // namespace snf
