// snf_bamindex.h - a BAM index (BAI, SAM specification 5.2; CSIv1 for any min_shift / depth) from the records an snf_bgzf_t holds after
// snf_bgzf_inflate: the inflated stream, d_rec_off and the member table; the host adds one column, the file offset of every member.
//
// Reference counterpart: the index pysam / htslib require behind `bam.fetch` (sniffles:172 check_index, leadprov.py:488) - htslib's
// hts_idx_push / bam_endpos / hts_reg2bin; the host form of the same rules is tests/bam_index_cases.py.  Kernels of
// snf_container.h: nothing else may include this header (the lane helpers, x_header and x_load_ops are snf_lanes.h's).
//
//   bai_span     per record: end (bam_endpos: pos + the summed lengths of M D N = X, pos + 1 when that is zero or the record is flagged
//                unmapped), bin (reg2bin(pos, end) for min_shift 14 / depth 5, recomputed - the record's own bin field is not read),
//                the virtual offsets of its first byte and of the byte behind it (member file offset << 16 | offset inside the member;
//                the member is the one that holds the byte: a binary search of out_off, so an empty member is never named), and a
//                sortedness word (BI_*) against its predecessor's refID / pos.  Wave form: a wave per record over a striding grid, the
//                lanes take the CIGAR BAI_STEP operations at a time (four per lane, one 16-byte load), a wave scan gives the sum.
//                Thread form (SNF_BAI_THREAD): a thread per record, the reference's loop.  Every read is bounded by the record's own
//                block_size and by the stream: a record whose n_cigar_op / l_read_name reach past its end leaves BI_TRUNCATED.
//   bai_linear   per mapped record: the 16-kb windows pos >> 14 .. (end - 1) >> 14 take the minimum of its start offset
//                (atomicMin on 64 bits in HBM); a wave's lanes take the windows, the thread form loops.
//   bai_flag     a record opens a chunk when its (refID, bin) differs from its predecessor's (the first record's predecessor comes in
//                with the carry); unplaced records (refID -1) open none.  Then rocPRIM's exclusive scan, bai_compact (the opening
//                records -> key refID << 32 | bin), a stable 64-bit radix sort (a bin's chunks stay in file order) and bai_table
//                (key, first byte of the chunk's first record, end of its last one).
//   csi_span / csi_linear   the same two bodies with the level scheme as run-time values of the view (snf_csi_run): the bin by
//                csi_reg2bin - a loop of `depth` rounds over the levels from the deepest upwards, 64-bit shifts and compares in
//                registers - and the windows at min_shift granularity.  The bai_* kernels are the instances with the literals 14 / 5;
//                flag, scan, compact, sort and table do not know the levels and serve both (a bin of depth 10 is below 2^31: the key
//                refID << 32 | bin holds it).
// No kernel here waits for another workgroup: what depends on a predecessor's result (the bin) is a kernel of its own.
#pragma once
#include "../../include/sniffles_amd.h"
#include "snf_lanes.h"

namespace snf {

enum { BI_OK = 0, BI_TRUNCATED = 1, BI_POS = 2, BI_REF = 3, BI_UNPLACED = 4, BI_REFID = 5 };
#define BAI_STEP 256      // CIGAR operations a wave takes per step (tests/bam_index_cases.py reads this literal)

struct BaiView {
  const uint8_t* stream; int64_t stream_len; const int64_t* rec_off; int64_t rel, n;      // record i starts at stream[rec_off[i] + rel]
  const snf_bgzf_member_t* mem; const int64_t* foff; int64_t n_mem;                      // foff[n_mem]: the file offset behind the run
  int64_t* end; uint32_t* bin; unsigned long long *vbeg, *vend; uint32_t* sorted;
  unsigned long long* err;               // [0] min over (record << 4 | BI_*), [1] the first unplaced record; ~0: none
  unsigned long long* lin; const int64_t* win_off; int32_t n_ref;      // lin[win_off[ref] + window]
  int64_t* flag; int64_t* run_idx; int64_t* run_start; unsigned long long* key; uint32_t* val;
  const unsigned long long* skey; const uint32_t* sval; unsigned long long* table; int64_t n_runs, n_placed;
  int32_t prev_ref, prev_pos; uint32_t prev_bin; int32_t have_prev;
  int32_t min_shift, depth;              // the CSI instances only: the level scheme of the run (the BAI instances never read them)
};

// SAM specification 5.3, min_shift 14 / depth 5; the interval is [beg, end)
SNF_HD uint32_t bai_reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// CSIv1, any min_shift / depth: the levels from the deepest upwards (bamindex.reg2bin); depth rounds on 64 bits, no memory access.  An
// interval that crosses 2^(min_shift + 3 depth) meets no level and falls to bin 0; with 14 / 5 this is bai_reg2bin value for value.
SNF_HD uint32_t csi_reg2bin(int64_t beg, int64_t end, int min_shift, int depth) {
  --end;
  int s = min_shift; int64_t t = ((1ll << (3 * depth)) - 1) / 7;
  for (int l = depth; l > 0; --l) {
    if (beg >> s == end >> s) return (uint32_t)(t + (beg >> s));
    s += 3; t -= 1ll << (3 * (l - 1));
  }
  return 0;
}
// stream position p in [0, stream_len] -> virtual offset: the last member whose output starts at or before p (behind the run: foff[n_mem])
SNF_HD unsigned long long bai_voff(const BaiView& v, int64_t p) {
  int64_t lo = 0, hi = v.n_mem;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    const int64_t off = mid == v.n_mem ? v.stream_len : v.mem[mid].out_off;
    if (off <= p) lo = mid; else hi = mid - 1;
  }
  const int64_t base = lo == v.n_mem ? v.stream_len : v.mem[lo].out_off;
  return ((unsigned long long)v.foff[lo] << 16) | (unsigned long long)(p - base);
}
SNF_HD void bai_error(const BaiView& v, int64_t rec, uint32_t code) { atomicMin(v.err, ((unsigned long long)rec << 4) | code); }

template <bool WAVE, bool CSI> SNF_HD void bai_span_rec(int64_t i, const BaiView& v) {
  const int lane = x_lane<WAVE>();
  const int64_t p = v.rec_off[i] + v.rel;
  int64_t end = 0; uint32_t bin = 0, code = BI_OK; unsigned long long vb = 0, ve = 0;
  if (p < 0 || p + 36 > v.stream_len) code = BI_TRUNCATED;
  else {
    uint32_t hd[6];
    x_header<WAVE>(v.stream + p, lane, hd);
    const int64_t bs = (int32_t)hd[0], rec_end = p + 4 + bs;
    const int32_t ref = (int32_t)hd[1], pos = (int32_t)hd[2];
    const int n_cig = (int)(hd[4] & 0xffffu); const uint32_t l_name = hd[3] & 0xffu, flag = hd[4] >> 16;
    if (bs < 32 || rec_end > v.stream_len || 36 + (int64_t)l_name + 4 * (int64_t)n_cig > 4 + bs) code = BI_TRUNCATED;
    else {
      const uint8_t* cig = v.stream + p + 36 + l_name;      // n_cig operations, all inside the record
      uint32_t sum = 0;
      if constexpr (WAVE) {
        for (int base = 0; base < n_cig; base += BAI_STEP) {
          uint32_t op[4] = {6u, 6u, 6u, 6u};
          x_load_ops<WAVE>(cig, n_cig, base, lane, op);
#pragma unroll
          for (int j = 0; j < 4; j++) if ((X_REFC >> (op[j] & 15u)) & 1u) sum += op[j] >> 4;
        }
        sum = x_bcast<WAVE>(x_incl_scan<WAVE>(sum, lane), 63);
      } else {
        for (int k = 0; k < n_cig; k++) { const uint32_t c = ld_u32(cig + 4 * (int64_t)k); if ((X_REFC >> (c & 15u)) & 1u) sum += c >> 4; }
      }
      end = (sum == 0 || (flag & 0x4u)) ? (int64_t)pos + 1 : (int64_t)pos + (int64_t)sum;
      if constexpr (CSI) bin = csi_reg2bin(pos, end, v.min_shift, v.depth); else bin = bai_reg2bin(pos, end);
      vb = bai_voff(v, p); ve = bai_voff(v, rec_end);
      // sortedness: against the record before (the first record's predecessor is the carry's)
      int32_t pref = v.prev_ref, ppos = v.prev_pos; bool have = v.have_prev != 0;
      if (i > 0) { const uint8_t* Q = v.stream + v.rec_off[i - 1] + v.rel; pref = (int32_t)ld_u32(Q + 4); ppos = (int32_t)ld_u32(Q + 8); have = true; }
      if (ref < -1 || ref >= v.n_ref) code = BI_REFID;
      else if (have && ref >= 0) {
        if (pref < 0) code = BI_UNPLACED;
        else if (ref < pref) code = BI_REF;
        else if (ref == pref && pos < ppos) code = BI_POS;
      }
    }
  }
  if (lane == 0) {
    v.end[i] = end; v.bin[i] = bin; v.vbeg[i] = vb; v.vend[i] = ve; v.sorted[i] = code;
    if (code) bai_error(v, i, code);
  }
}
__global__ void __launch_bounds__(64) bai_span_wave(const BaiView v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x; i < n; i += (int64_t)gridDim.x) bai_span_rec<true, false>(i, v);
}
SNF_HD void bai_span_thread_body(int64_t i, const BaiView& v) { bai_span_rec<false, false>(i, v); }
SNF_KERNEL(bai_span_thread, BaiView)
__global__ void __launch_bounds__(64) csi_span_wave(const BaiView v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x; i < n; i += (int64_t)gridDim.x) bai_span_rec<true, true>(i, v);
}
SNF_HD void csi_span_thread_body(int64_t i, const BaiView& v) { bai_span_rec<false, true>(i, v); }
SNF_KERNEL(csi_span_thread, BaiView)

template <bool WAVE, bool CSI> SNF_HD void bai_linear_rec(int64_t i, const BaiView& v) {
  const uint32_t st = v.sorted[i];
  if (st == BI_TRUNCATED || st == BI_REFID) return;
  const uint8_t* R = v.stream + v.rec_off[i] + v.rel;
  const int32_t ref = (int32_t)ld_u32(R + 4), pos = (int32_t)ld_u32(R + 8);
  if (ref < 0 || ((ld_u32(R + 16) >> 16) & 0x4u)) return;
  const int64_t end = v.end[i], nw = v.win_off[ref + 1] - v.win_off[ref];
  const int sh = CSI ? v.min_shift : 14;      // (win_off is the caller's table at the same shift)
  const int64_t w0 = (pos > 0 ? (int64_t)pos : 0) >> sh;
  int64_t w1 = ((end > 1 ? end : 1) - 1) >> sh;
  if (w1 >= nw) w1 = nw - 1;      // (a record beyond the header's length of its reference: the table ends there)
  const unsigned long long vb = v.vbeg[i];
  unsigned long long* L = v.lin + v.win_off[ref];
  for (int64_t w = w0 + x_lane<WAVE>(); w <= w1; w += WAVE ? 64 : 1) atomicMin(&L[w], vb);
}
__global__ void __launch_bounds__(64) bai_linear_wave(const BaiView v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x; i < n; i += (int64_t)gridDim.x) bai_linear_rec<true, false>(i, v);
}
SNF_HD void bai_linear_thread_body(int64_t i, const BaiView& v) { bai_linear_rec<false, false>(i, v); }
SNF_KERNEL(bai_linear_thread, BaiView)
__global__ void __launch_bounds__(64) csi_linear_wave(const BaiView v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x; i < n; i += (int64_t)gridDim.x) bai_linear_rec<true, true>(i, v);
}
SNF_HD void csi_linear_thread_body(int64_t i, const BaiView& v) { bai_linear_rec<false, true>(i, v); }
SNF_KERNEL(csi_linear_thread, BaiView)

// ---- chunk runs: flag, (scan), compact, (sort), table -------------------------------------------------------------------
SNF_HD void bai_flag_body(int64_t i, const BaiView& v) {      // n + 1 threads: flag[n] = 0 so that run_idx[n] is the number of runs
  int64_t f = 0;
  if (i < v.n && v.sorted[i] != BI_TRUNCATED) {
    const int32_t ref = (int32_t)ld_u32(v.stream + v.rec_off[i] + v.rel + 4);
    if (ref < 0) atomicMin(v.err + 1, (unsigned long long)i);
    else {
      int32_t pref = v.prev_ref; uint32_t pbin = v.prev_bin; bool have = v.have_prev != 0;
      if (i > 0) { pref = (int32_t)ld_u32(v.stream + v.rec_off[i - 1] + v.rel + 4); pbin = v.bin[i - 1]; have = true; }
      f = (!have || pref != ref || pbin != v.bin[i]) ? 1 : 0;
    }
  }
  v.flag[i] = f;
}
SNF_KERNEL(bai_flag, BaiView)
SNF_HD void bai_compact_body(int64_t i, const BaiView& v) {
  if (!v.flag[i]) return;
  const int64_t r = v.run_idx[i];
  const int32_t ref = (int32_t)ld_u32(v.stream + v.rec_off[i] + v.rel + 4);
  v.run_start[r] = i; v.key[r] = ((unsigned long long)(uint32_t)ref << 32) | v.bin[i]; v.val[r] = (uint32_t)r;
}
SNF_KERNEL(bai_compact, BaiView)
SNF_HD void bai_table_body(int64_t r, const BaiView& v) {      // sorted run r: (key, beg, end)
  const int64_t j = (int64_t)v.sval[r];
  const int64_t first = v.run_start[j], last = (j + 1 < v.n_runs ? v.run_start[j + 1] : v.n_placed) - 1;
  v.table[3 * r] = v.skey[r]; v.table[3 * r + 1] = v.vbeg[first]; v.table[3 * r + 2] = v.vend[last];
}
SNF_KERNEL(bai_table, BaiView)

}  // namespace snf
