// snf_genotype.h - force calling (--genotype-vcf): GenotypeTask.execute of the reference (parallel.py:299-372) on the device.
//
// The match: every target SV of the input VCF takes the closest candidate of its type within the merge gates.  The reference
// files the targets into a 5-kb bin table (a target near a bin edge also into the neighbour bin) and lets every candidate look
// into the bin of its own position; restated per target t:
//   * t is visible in bin b0 = t.pos / 5000, in b0 - 1 iff t.pos % 5000 < 500 and in b0 + 1 iff t.pos % 5000 > 4500
//   * candidate c sees t iff the types are equal and c.pos / 5000 is one of those bins (SINGLE_* candidates and targets whose
//     type is not one of sv.TYPES take no part; bin -1 holds nobody) - a bin rule, not a distance rule
//   * BND: dist = |dpos|, ok iff dist <= cluster_merge_bnd and the mate contigs are equal
//     else: dist = |dpos| + ||t.svlen| - |c.svlen||, minlen = min(|t.svlen|, |c.svlen|), ok iff minlen > 0 and
//     (double)dist <= (double)combine_match * sqrt((double)minlen) (IEEE square root, one fp64 multiply) and dist <= combine_match_max
//   * the smallest dist among the ok candidates wins, the earliest in candidate order among equals
// Device form: a key (type, bin) per candidate (gt_keys), a stable radix sort of (key, candidate index), then one wave per
// target: the bounds of each visible bin by binary search in the sorted keys, the lanes stride over the bin's candidates, a
// wave-min over the 64-bit value (dist << 32 | candidate index), lane 0 stores.  gt_match_thread is the thread-per-target form
// of the same body.  The candidate columns are read through a stride, so that the snf_call_t records of a batch serve as they lie.
//
// The genotype: what VCF.rewrite_genotype prints for a target - the matched candidate's genotype when it has one, else the
// reference-allele genotype from the coverage samples of the target (parallel.py:355-366).
#pragma once
#include "snf_rt.h"
#include "../../include/sniffles_amd.h"

namespace snf {

constexpr int64_t GT_BINSIZE = 5000, GT_BINEDGE = 500;
constexpr unsigned GT_BIN_BITS = 20, GT_KEY_BITS = 24;             // pos < 2^31: bin < 2^19; type < 16
constexpr uint32_t GT_KEY_DROPPED = (1u << GT_KEY_BITS) - 1;        // sorts behind every key a target asks for
constexpr int GT_WAVES = 4;                                         // waves (= targets in flight) per workgroup of gt_match_wave

struct GtMatchView {
  const int32_t *c_svtype, *c_pos, *c_svlen, *c_mate; int64_t c_stride, nc;   // candidates: element i at [i * c_stride]
  const int32_t *t_svtype, *t_pos, *t_svlen, *t_mate; int64_t nt;             // targets
  uint32_t *key_in, *key_out, *idx_in, *idx_out;                              // [nc] each: (key, candidate) before / behind the sort
  int32_t *out_best, *out_dist;                                               // [nt]
  int32_t merge_bnd, combine_match, combine_match_max;
};

SNF_HD void gt_keys_body(int64_t i, const GtMatchView& v) {
  const int32_t t = v.c_svtype[i * v.c_stride], p = v.c_pos[i * v.c_stride];
  const bool in = t >= SNF_INS && t <= SNF_BND && p >= 0;
  v.key_in[i] = in ? ((uint32_t)t << GT_BIN_BITS | (uint32_t)(p / GT_BINSIZE)) : GT_KEY_DROPPED;
  v.idx_in[i] = (uint32_t)i;
}

// first position in the sorted keys that is not below `key`
SNF_HD int64_t gt_lower_bound(const uint32_t* keys, int64_t n, uint32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}

template <bool WAVE>
SNF_HD void gt_match_run(int64_t t, const GtMatchView& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
#else
  const int lane = 0;
#endif
  const int64_t step = WAVE ? 64 : 1;
  const int64_t none = INT64_MAX;
  const int32_t tt = v.t_svtype[t];
  int64_t key = none;
  if (tt >= SNF_INS && tt <= SNF_BND) {
    const int64_t tpos = v.t_pos[t], tl = v.t_svlen[t], tlen = tl < 0 ? -tl : tl;
    const int32_t tmate = v.t_mate[t];
    const int64_t b0 = tpos / GT_BINSIZE, m = ((tpos % GT_BINSIZE) + GT_BINSIZE) % GT_BINSIZE;
    for (int k = 0; k < 3; k++) {
      const int64_t b = k == 0 ? b0 : (k == 1 ? b0 - 1 : b0 + 1);
      if ((k == 1 && !(m < GT_BINEDGE)) || (k == 2 && !(m > GT_BINSIZE - GT_BINEDGE))) continue;
      if (b < 0 || b >= ((int64_t)1 << GT_BIN_BITS)) continue;
      const uint32_t bk = (uint32_t)tt << GT_BIN_BITS | (uint32_t)b;
      const int64_t lo = gt_lower_bound(v.key_out, v.nc, bk), hi = gt_lower_bound(v.key_out, v.nc, bk + 1);
      for (int64_t i = lo + lane; i < hi; i += step) {
        const int64_t c = v.idx_out[i];
        const int64_t dp = tpos - (int64_t)v.c_pos[c * v.c_stride];
        int64_t dist = dp < 0 ? -dp : dp;
        bool ok;
        if (tt == SNF_BND) {
          ok = dist <= (int64_t)v.merge_bnd && v.c_mate[c * v.c_stride] == tmate;
        } else {
          const int64_t cl = v.c_svlen[c * v.c_stride], clen = cl < 0 ? -cl : cl, dl = tlen - clen;
          dist += dl < 0 ? -dl : dl;
          const int64_t minlen = tlen < clen ? tlen : clen;
          ok = minlen > 0 && (double)dist <= (double)v.combine_match * sqrt((double)minlen) && dist <= (int64_t)v.combine_match_max;
        }
        if (ok) {                        // (dist < 2^31 from here: it passed a gate that is an int32)
          const int64_t kk = dist << 32 | c;
          if (kk < key) key = kk;
        }
      }
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  if (WAVE) {
    for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor((long long)key, d, 64); if (o < key) key = o; }
  }
#endif
  if (lane == 0) {
    v.out_best[t] = key == none ? -1 : (int32_t)(key & 0xffffffffll);
    v.out_dist[t] = key == none ? 0 : (int32_t)(key >> 32);
  }
}

// ---- the genotype a target is written with (VCF.rewrite_genotype over GenotypeTask.execute's tail, parallel.py:360-366)
struct GtTupleView {
  const snf_call_t* cand; int64_t nc;      // the task's candidates (finalized records)
  const int32_t* best;                     // [n] index into cand, -1
  const int32_t* cov;                      // [5n] upstream, start, center, end, downstream; SNF_NONE_I32: unset
  const int32_t* n_valid;                  // CovCalls::n_valid: targets behind [0] were not annotated (BND before any other call)
  int32_t* gt;                             // [8n] a, b, GQ, DR, DV, hp, ps, source (enum snf_gtsrc)
  int32_t* depth;                          // [n] round(mean(start, center, end over those that are set)); SNF_NONE_I32: none is set
  int32_t* no_sample;                      // [1] set when a target has no sample at all (the reference returns None for the task)
  int64_t n;
};

// Python's round(sum / cnt) for cnt in 1..3 in integers: halves go to the even neighbour (cnt == 2), thirds to the nearest
SNF_HD int64_t gt_round_mean(int64_t sum, int cnt) {
  if (cnt == 1) return sum;
  int64_t q = sum / cnt, r = sum % cnt;
  if (r < 0) { r += cnt; q -= 1; }        // floor division
  if (cnt == 2) return r == 0 ? q : ((q & 1) ? q + 1 : q);
  return r == 2 ? q + 1 : q;
}

SNF_HD void gt_tuple_body(int64_t i, const GtTupleView& q) {
  int32_t* g = q.gt + 8 * i;
  int64_t sum = 0; int cnt = 0;
  for (int k = 1; k <= 3; k++) { const int32_t c = q.cov[5 * i + k]; if (c != SNF_NONE_I32) { sum += c; cnt++; } }
  if (cnt == 0 && i < q.n_valid[0]) atomic_or_i32(q.no_sample, 1);
  const int64_t depth = cnt ? gt_round_mean(sum, cnt) : 0;
  q.depth[i] = cnt ? (int32_t)depth : SNF_NONE_I32;
  const int32_t b = q.best[i];
  if (b >= 0 && (int64_t)b < q.nc && q.cand[b].gt_set) {
    const snf_call_t& c = q.cand[b];
    g[0] = c.gt_a; g[1] = c.gt_b; g[2] = c.gt_gq; g[3] = c.gt_dr; g[4] = c.gt_dv; g[5] = c.gt_hp; g[6] = c.gt_ps; g[7] = SNF_GTSRC_MATCH;
  } else {
    g[0] = g[1] = g[2] = g[4] = 0; g[3] = depth > 0 ? (int32_t)depth : 0; g[5] = g[6] = -1;
    g[7] = depth > 0 ? SNF_GTSRC_DEPTH : SNF_GTSRC_NONE;
  }
}

// The launch chain of the match on `st` (defined once, in the unit that holds the combine kernels): keys, sort, match.
// `tmp`: gt_match_tmp_bytes(nc) bytes of device scratch for the sort.  form 0: one wave per target, 1: one thread per target;
// max_grid <= 0: no cap on the workgroups of the match (the kernels stride when capped).  Returns the grid of the match.
size_t gt_match_tmp_bytes(int64_t nc);
int64_t gt_match_enqueue(const GtMatchView& v, void* tmp, size_t tmp_bytes, hipStream_t st, int32_t max_grid, int form);

}  // namespace snf
