// snf_container.h - the container layer's five handles, host side (kernels: snf_bgzf.h, snf_bamindex.h, snf_deflate.h, snf_fasta.h,
// snf_vcftext.h): each a struct, its do_* functions (they throw snf::Error) and its extern "C" block behind the C boundary of
// snf_devmem.h.  Definitions: ONE unit includes this file (snf_extract.hip, at its end); it shares only snf_lanes.h and snf_devmem.h
// with the extraction, which takes the inflated records through plain device pointers (snf_extract_attach_device).
#pragma once
#include "../../include/sniffles_amd.h"
#include "snf_lanes.h"
#include "snf_devmem.h"
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "snf_bgzf.h"
#include "snf_bamindex.h"
#include "snf_deflate.h"
#include "snf_fasta.h"
#include "snf_vcftext.h"
using namespace snf;

// ========================================================================== BGZF inflate + record chain: host side ====
struct snf_bgzf {
  int device = 0;
  std::vector<void*> dev;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* d_stream = nullptr; int64_t* d_rec_off = nullptr;
  std::vector<int64_t> h_rec_off; std::vector<uint32_t> h_heads; std::vector<uint8_t> h_names;
  snf_bgzf_result_t res{};
  bool have = false;
  // what snf_bai_run takes from the last inflate, and its host tables
  const snf_bgzf_member_t* d_mem = nullptr; int64_t n_mem = 0, origin = 0, stream_pos = 0;
  std::vector<void*> bai_dev;
  hipEvent_t bev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // span | linear | flag + scan | compact + sort + table
  std::vector<int64_t> b_end, b_win; std::vector<uint32_t> b_bin; std::vector<uint64_t> b_vbeg, b_vend, b_runs, b_min;
};

namespace {
thread_local std::string g_zerr, g_berr;

void do_bgzf_inflate(snf_bgzf* z, const uint8_t* comp, int64_t comp_len, const snf_bgzf_member_t* mem, int64_t n_mem, const snf_bam_carry_t* cin) {
  if (comp_len < 0 || n_mem < 0 || (comp_len && !comp) || (n_mem && !mem) || !cin) snf::fail("snf_bgzf_inflate: null argument");
  if (cin->skip < 0 || cin->skip >= (1ll << 36) || cin->count < 0 || cin->n_part > 3 || (cin->n_part && cin->skip)) snf::fail("snf_bgzf_inflate: malformed carry");
  int64_t total = 0;
  for (int64_t m = 0; m < n_mem; m++) {
    const snf_bgzf_member_t& b = mem[m];
    if (b.payload_off < 0 || b.payload_off + (int64_t)b.payload_len > comp_len) snf::fail("BGZF member " + std::to_string(m) + ": payload outside the compressed bytes");
    if (b.isize > BZ_WIN) snf::fail("BGZF member " + std::to_string(m) + ": ISIZE above 65536");
    if (b.out_off != total) snf::fail("BGZF member " + std::to_string(m) + ": out_off is not the exclusive sum of ISIZE");
    total += b.isize;
  }
  const BgzfKnobs k;
  x_release(z->dev); x_release(z->bai_dev);
  z->have = false; z->d_stream = nullptr; z->d_rec_off = nullptr; z->d_mem = nullptr;
  const int64_t rec_cap = total / 36 + 2;      // a record is at least 36 bytes; one more for the end of the run
  uint8_t* d_comp; snf_bgzf_member_t* d_mem; uint32_t* d_status; unsigned long long* d_carry; uint32_t* d_misc;
  try {
    d_comp = x_up(z->dev, comp, (size_t)comp_len, 16);
    d_mem = x_up(z->dev, mem, (size_t)n_mem);
    z->d_stream = x_alloc<uint8_t>(z->dev, (size_t)total, 64);
    z->d_rec_off = x_alloc<int64_t>(z->dev, (size_t)rec_cap);
    d_status = x_alloc<uint32_t>(z->dev, (size_t)n_mem);
    d_carry = x_alloc<unsigned long long>(z->dev, 2 * (size_t)n_mem + 4);      // [2 (n_mem + 1)] .. : the error word
    d_misc = x_alloc<uint32_t>(z->dev, 4);                                     // [0] ticket, [1] longest l_read_name
  } catch (const snf::Error& e) {
    x_release(z->dev);
    snf::fail("the BAM's " + std::to_string((long long)total) + " inflated bytes (and " + std::to_string((long long)comp_len) +
              " compressed) do not fit the free device memory: " + e.msg);
  }
  SNF_HIP(hipMemset(z->d_stream + total, 0, 64));
  for (hipEvent_t& e : z->ev) if (!e) SNF_HIP(hipEventCreate(&e));
  // ---- inflate
  BgzfView bv{d_comp, d_mem, n_mem, z->d_stream, d_status};
  SNF_HIP(hipEventRecord(z->ev[0], 0));
  if (n_mem) {
    if (k.thread_form) hipLaunchKernelGGL(bgzf_inflate_thread, dim3((unsigned)((n_mem + 63) / 64)), dim3(64), 0, 0, bv, n_mem);
    else hipLaunchKernelGGL(bgzf_inflate_wave, dim3((unsigned)std::min<int64_t>(n_mem, k.grid_cap)), dim3(64), 0, 0, bv, n_mem);
  }
  SNF_HIP(hipEventRecord(z->ev[1], 0));
  std::vector<uint32_t> status((size_t)n_mem);
  x_d2h(status.data(), d_status, (size_t)n_mem * 4);
  for (int64_t m = 0; m < n_mem; m++)
    if (status[(size_t)m]) snf::fail("BGZF member " + std::to_string(m) + ": " + BZ_TEXT[status[(size_t)m] < 8 ? status[(size_t)m] : 4]);
  // ---- record chain
  const unsigned long long none = ~0ull;
  unsigned long long* d_err = d_carry + 2 * (size_t)n_mem + 2;
  SNF_HIP(hipMemset(d_carry, 0, (2 * (size_t)n_mem + 4) * 8));
  SNF_HIP(hipMemset(d_misc, 0, 16));
  {
    const unsigned long long c0[2] = {BC_VALID | (unsigned long long)cin->skip << 26 |
                                      ((unsigned long long)cin->part[0] | (unsigned long long)cin->part[1] << 8 | (unsigned long long)cin->part[2] << 16) << 2 | cin->n_part,
                                      BC_VALID | (unsigned long long)cin->count};
    x_h2d(d_carry, c0, 16); x_h2d(d_err, &none, 8);
  }
  ChainView cv{z->d_stream, d_mem, n_mem, z->d_rec_off, rec_cap - 1, d_carry, d_misc, d_err, cin->stream_pos, cin->origin, cin->count, 1u << 22};
  SNF_HIP(hipEventRecord(z->ev[2], 0));
  if (n_mem) hipLaunchKernelGGL(bam_chain, dim3((unsigned)n_mem), dim3(64), 0, 0, cv, n_mem);
  SNF_HIP(hipEventRecord(z->ev[3], 0));
  unsigned long long cout[4] = {0, 0, 0, 0};
  x_d2h(cout, d_carry + 2 * (size_t)n_mem, 24);
  if (cout[2] != none) {
    const int code = (int)(cout[2] & 15);
    if (code == BC_BLOCK_SIZE) snf::fail("truncated BAM record at byte " + std::to_string((long long)(cout[2] >> 4)));
    snf::fail(code == BC_TIMEOUT ? "record chain: a segment's predecessor never published its carry (segment at byte " + std::to_string((long long)(cout[2] >> 4)) + ")"
                                 : "record chain: more records than the offset table holds");
  }
  snf_bgzf_result_t& r = z->res;
  r = snf_bgzf_result_t{};
  r.carry.skip = (int64_t)((cout[0] & ~BC_VALID) >> 26);
  r.carry.n_part = (uint8_t)(cout[0] & 3); for (int b = 0; b < 3; b++) r.carry.part[b] = (uint8_t)(cout[0] >> (2 + 8 * b));
  r.carry.count = (int64_t)(cout[1] & ~(BC_VALID | BC_ABORT));
  r.carry.stream_pos = cin->stream_pos + total; r.carry.origin = cin->origin;
  const int64_t n = r.carry.count - cin->count;
  const int64_t end = cin->stream_pos + total - cin->origin;
  x_h2d(z->d_rec_off + n, &end, 8);
  // ---- heads, then the names at the width the heads give
  z->h_rec_off.assign((size_t)n + 1, 0); z->h_heads.assign((size_t)n * 6 + 1, 0);
  x_d2h(z->h_rec_off.data(), z->d_rec_off, ((size_t)n + 1) * 8);
  uint32_t width = 0;
  if (n) {
    uint32_t* d_heads = x_alloc<uint32_t>(z->dev, (size_t)n * 6);
    HeadsView hv{z->d_stream, total, z->d_rec_off, cin->origin - cin->stream_pos, d_heads, nullptr, d_misc + 1, 0, 0};
    hipLaunchKernelGGL(bam_heads, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, hv, n);
    x_d2h(&width, d_misc + 1, 4);
    x_d2h(z->h_heads.data(), d_heads, (size_t)n * 24);
    z->h_names.assign((size_t)n * width + 1, 0);
    if (width) {
      hv.names = x_alloc<uint8_t>(z->dev, (size_t)n * width); hv.width = (int32_t)width; hv.phase = 1;
      hipLaunchKernelGGL(bam_heads, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, hv, n);
      x_d2h(z->h_names.data(), hv.names, (size_t)n * width);
    }
  } else z->h_names.assign(1, 0);
  SNF_HIP(hipDeviceSynchronize());
  SNF_HIP(hipEventElapsedTime(&r.ms_inflate, z->ev[0], z->ev[1])); SNF_HIP(hipEventElapsedTime(&r.ms_chain, z->ev[2], z->ev[3]));
  r.stream_len = total; r.n_records = n; r.rec_off = z->h_rec_off.data(); r.heads = z->h_heads.data(); r.names = z->h_names.data();
  r.name_width = (int32_t)width; r.device = z->device; r.d_stream = z->d_stream; r.d_rec_off = z->d_rec_off;
  z->d_mem = d_mem; z->n_mem = n_mem; z->origin = cin->origin; z->stream_pos = cin->stream_pos;
  z->have = true;
}

// ---- BAM index of the run (snf_bamindex.h)
// `csi`: the level scheme comes from min_shift / depth (snf_csi_run, the csi_* instances); otherwise the literals 14 / 5
void do_bai_run(snf_bgzf* z, const int64_t* foff, const snf_bai_carry_t* cin, snf_bai_run_result_t* out, bool csi = false, int32_t min_shift = 14,
                int32_t depth = 5) {
  if (!foff || !cin || !out) snf::fail("snf_bai_run: null argument");
  if (!z->have) snf::fail("snf_bai_run before a successful snf_bgzf_inflate");
  if (cin->n_ref < 0 || !cin->win_off) snf::fail("snf_bai_run: window table missing");
  for (int32_t r = 0; r < cin->n_ref; r++) if (cin->win_off[r + 1] < cin->win_off[r] || cin->win_off[0] != 0) snf::fail("snf_bai_run: win_off is not ascending from 0");
  for (int64_t m = 0; m < z->n_mem; m++) if (foff[m] < 0 || foff[m + 1] < foff[m] || foff[m + 1] >= (1ll << 48)) snf::fail("snf_bai_run: member file offsets malformed");
  const BaiKnobs k;
  x_release(z->bai_dev);
  std::vector<void*>& pool = z->bai_dev;
  const snf_bgzf_result_t& zr = z->res;
  const int64_t n = zr.n_records - (zr.carry.skip != 0 && zr.n_records > 0 ? 1 : 0);      // the end of the run cuts the last record
  const int64_t n_win = cin->win_off[cin->n_ref];
  const size_t N1 = (size_t)n + 1;
  BaiView v{};
  v.stream = z->d_stream; v.stream_len = zr.stream_len; v.rec_off = z->d_rec_off; v.rel = z->origin - z->stream_pos; v.n = n;
  v.mem = z->d_mem; v.n_mem = z->n_mem; v.foff = x_up(pool, foff, (size_t)z->n_mem + 1);
  v.end = x_alloc<int64_t>(pool, N1); v.bin = x_alloc<uint32_t>(pool, N1); v.vbeg = x_alloc<unsigned long long>(pool, N1);
  v.vend = x_alloc<unsigned long long>(pool, N1); v.sorted = x_alloc<uint32_t>(pool, N1);
  v.err = x_alloc<unsigned long long>(pool, 2);
  v.lin = x_alloc<unsigned long long>(pool, (size_t)n_win); v.win_off = x_up(pool, cin->win_off, (size_t)cin->n_ref + 1); v.n_ref = cin->n_ref;
  v.flag = x_alloc<int64_t>(pool, N1); v.run_idx = x_alloc<int64_t>(pool, N1);
  v.prev_ref = cin->prev_ref; v.prev_pos = cin->prev_pos; v.prev_bin = cin->prev_bin; v.have_prev = cin->have_prev;
  v.min_shift = min_shift; v.depth = depth;
  const unsigned long long none[2] = {~0ull, ~0ull};
  x_h2d(v.err, none, 16);
  SNF_HIP(hipMemset(v.lin, 0xff, (size_t)(n_win ? n_win : 1) * 8));
  for (hipEvent_t& e : z->bev) if (!e) SNF_HIP(hipEventCreate(&e));
  const unsigned grid_w = (unsigned)std::min<int64_t>(n > 0 ? n : 1, k.grid_cap), grid_t = (unsigned)((n + 255) / 256);
  // (every bracket holds launches only: the copies to the host and the host's waits lie between the brackets)
  SNF_HIP(hipEventRecord(z->bev[0], 0));
  if (n) {
    if (csi) {
      if (k.thread_form) hipLaunchKernelGGL(csi_span_thread, dim3(grid_t), dim3(256), 0, 0, v, n);
      else hipLaunchKernelGGL(csi_span_wave, dim3(grid_w), dim3(64), 0, 0, v, n);
    } else if (k.thread_form) hipLaunchKernelGGL(bai_span_thread, dim3(grid_t), dim3(256), 0, 0, v, n);
    else hipLaunchKernelGGL(bai_span_wave, dim3(grid_w), dim3(64), 0, 0, v, n);
    SNF_HIP(hipGetLastError());
  }
  SNF_HIP(hipEventRecord(z->bev[1], 0));
  unsigned long long err[2] = {~0ull, ~0ull};
  x_d2h(err, v.err, 16);
  z->b_end.assign(N1, 0); z->b_bin.assign(N1, 0); z->b_vbeg.assign(N1, 0); z->b_vend.assign(N1, 0);
  x_d2h(z->b_end.data(), v.end, (size_t)n * 8); x_d2h(z->b_bin.data(), v.bin, (size_t)n * 4);
  x_d2h(z->b_vbeg.data(), v.vbeg, (size_t)n * 8); x_d2h(z->b_vend.data(), v.vend, (size_t)n * 8);
  if (err[0] != ~0ull) {
    const int64_t rec = (int64_t)(err[0] >> 4); const int code = (int)(err[0] & 15);
    x_release(pool);
    if (code == BI_TRUNCATED) snf::fail("truncated BAM record at byte " + std::to_string((long long)(zr.rec_off[rec] + z->origin)));
    const uint32_t* h = zr.heads + 6 * rec;
    const std::string at = "BAM not coordinate-sorted: record " + std::to_string((long long)(cin->count + rec)) + " (reference " +
                           std::to_string((int32_t)h[1]) + ", position " + std::to_string((int32_t)h[2]) + ")";
    snf::fail(at + (code == BI_POS ? " lies before its predecessor's position" : code == BI_REF ? " follows a record of a later reference"
                    : code == BI_UNPLACED ? " follows an unplaced record" : " names a reference the header does not have"));
  }
  // ---- linear index
  size_t scan_need = 0;
  SNF_HIP(rocprim::exclusive_scan(nullptr, scan_need, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  void* scan_tmp = x_alloc<uint8_t>(pool, scan_need);
  SNF_HIP(hipEventRecord(z->bev[2], 0));
  if (n) {
    if (csi) {
      if (k.thread_form) hipLaunchKernelGGL(csi_linear_thread, dim3(grid_t), dim3(256), 0, 0, v, n);
      else hipLaunchKernelGGL(csi_linear_wave, dim3(grid_w), dim3(64), 0, 0, v, n);
    } else if (k.thread_form) hipLaunchKernelGGL(bai_linear_thread, dim3(grid_t), dim3(256), 0, 0, v, n);
    else hipLaunchKernelGGL(bai_linear_wave, dim3(grid_w), dim3(64), 0, 0, v, n);
    SNF_HIP(hipGetLastError());
  }
  SNF_HIP(hipEventRecord(z->bev[3], 0));
  // ---- chunks: flag, scan | the number of chunks to the host | compact, sort, table
  hipLaunchKernelGGL(bai_flag, dim3((unsigned)((N1 + 255) / 256)), dim3(256), 0, 0, v, (int64_t)N1);
  SNF_HIP(hipGetLastError());
  SNF_HIP(rocprim::exclusive_scan(scan_tmp, scan_need, (const int64_t*)v.flag, v.run_idx, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  SNF_HIP(hipEventRecord(z->bev[4], 0));
  int64_t n_runs = 0;
  x_d2h(&n_runs, v.run_idx + n, 8);
  x_d2h(err, v.err, 16);
  v.n_runs = n_runs; v.n_placed = err[1] == ~0ull ? n : (int64_t)err[1];
  z->b_runs.assign((size_t)n_runs * 3 + 1, 0);
  int64_t head_n = 0;
  if (n_runs) {
    const size_t R = (size_t)n_runs;
    v.run_start = x_alloc<int64_t>(pool, R); v.key = x_alloc<unsigned long long>(pool, R); v.val = x_alloc<uint32_t>(pool, R);
    unsigned long long* skey = x_alloc<unsigned long long>(pool, R); uint32_t* sval = x_alloc<uint32_t>(pool, R);
    v.table = x_alloc<unsigned long long>(pool, 3 * R);
    size_t need = 0;
    SNF_HIP(rocprim::radix_sort_pairs(nullptr, need, (const unsigned long long*)v.key, skey, (const uint32_t*)v.val, sval, R, 0u, 64u, 0));
    void* tmp = x_alloc<uint8_t>(pool, need);
    SNF_HIP(hipEventRecord(z->bev[5], 0));
    hipLaunchKernelGGL(bai_compact, dim3(grid_t), dim3(256), 0, 0, v, n);
    SNF_HIP(hipGetLastError());
    SNF_HIP(rocprim::radix_sort_pairs(tmp, need, (const unsigned long long*)v.key, skey, (const uint32_t*)v.val, sval, R, 0u, 64u, 0));
    v.skey = skey; v.sval = sval;
    hipLaunchKernelGGL(bai_table, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, 0, v, n_runs);
    SNF_HIP(hipGetLastError());
    SNF_HIP(hipEventRecord(z->bev[6], 0));
    x_d2h(z->b_runs.data(), v.table, R * 24);
    x_d2h(&head_n, v.run_start, 8);      // records in front of the first chunk this run opens: they continue the carry's
  } else head_n = v.n_placed;
  // ---- the windows touched
  std::vector<uint64_t> lin((size_t)n_win + 1);
  x_d2h(lin.data(), v.lin, (size_t)n_win * 8);
  SNF_HIP(hipDeviceSynchronize());
  z->b_win.clear(); z->b_min.clear();
  for (int64_t w = 0; w < n_win; w++) if (lin[(size_t)w] != ~0ull) { z->b_win.push_back(w); z->b_min.push_back(lin[(size_t)w]); }
  const int64_t n_touched = (int64_t)z->b_win.size();
  z->b_win.push_back(0); z->b_min.push_back(0);
  snf_bai_run_result_t r{};
  SNF_HIP(hipEventElapsedTime(&r.ms_span, z->bev[0], z->bev[1])); SNF_HIP(hipEventElapsedTime(&r.ms_linear, z->bev[2], z->bev[3]));
  SNF_HIP(hipEventElapsedTime(&r.ms_runs, z->bev[3], z->bev[4]));
  if (n_runs) { float ms2 = 0; SNF_HIP(hipEventElapsedTime(&ms2, z->bev[5], z->bev[6])); r.ms_runs += ms2; }
  r.n_records = n; r.end = z->b_end.data(); r.bin = z->b_bin.data(); r.vbeg = z->b_vbeg.data(); r.vend = z->b_vend.data();
  r.n_runs = n_runs; r.runs = z->b_runs.data(); r.head_n = head_n; r.head_end = head_n ? z->b_vend[(size_t)head_n - 1] : 0;
  r.n_windows = n_touched; r.win_index = z->b_win.data(); r.win_min = z->b_min.data();
  r.carry = *cin; r.carry.count = cin->count + n;
  r.carry.win_off = nullptr;      // (the caller's table: not handed back)
  if (n) {
    const uint32_t* h = zr.heads + 6 * (n - 1);
    r.carry.have_prev = 1; r.carry.prev_ref = (int32_t)h[1]; r.carry.prev_pos = (int32_t)h[2]; r.carry.prev_bin = z->b_bin[(size_t)n - 1];
  }
  x_release(pool);
  *out = r;
}
}  // namespace

extern "C" {
const char* snf_bgzf_last_error(void) { return g_zerr.c_str(); }
int snf_bgzf_create(int device, snf_bgzf_t** out) {
  if (!out) { g_zerr = "snf_bgzf_create: null argument"; return 1; }
  if (c_create(g_zerr, device, "BGZF")) return 1;
  snf_bgzf* z = new snf_bgzf();
  z->device = device;
  *out = z;
  return 0;
}
int snf_bgzf_inflate(snf_bgzf_t* z, const uint8_t* compressed, int64_t compressed_len, const snf_bgzf_member_t* members, int64_t n_members,
                     const snf_bam_carry_t* carry_in) {
  if (!z) { g_zerr = "null handle"; return 1; }
  return c_entry(g_zerr, z->device, [&] { do_bgzf_inflate(z, compressed, compressed_len, members, n_members, carry_in); });
}
int snf_bgzf_result(snf_bgzf_t* z, snf_bgzf_result_t* out) {
  if (!z || !out) { g_zerr = "null argument"; return 1; }
  if (!z->have) { g_zerr = "snf_bgzf_result before a successful snf_bgzf_inflate"; return 1; }
  *out = z->res;
  return 0;
}
int snf_bgzf_read_stream(snf_bgzf_t* z, int64_t off, int64_t len, uint8_t* dst) {
  if (!z || (len && !dst)) { g_zerr = "null argument"; return 1; }
  if (!z->have) { g_zerr = "snf_bgzf_read_stream before a successful snf_bgzf_inflate"; return 1; }
  if (off < 0 || len < 0 || off + len > z->res.stream_len) { g_zerr = "snf_bgzf_read_stream: range outside the stream"; return 1; }
  return c_entry(g_zerr, z->device, [&] { x_d2h(dst, z->d_stream + off, (size_t)len); });
}
int snf_bai_run(snf_bgzf_t* z, const int64_t* member_file_off, const snf_bai_carry_t* in, snf_bai_run_result_t* out) {
  if (!z) { g_berr = "null handle"; return 1; }
  return c_entry(g_berr, z->device, [&] { do_bai_run(z, member_file_off, in, out); });
}
int snf_csi_run(snf_bgzf_t* z, const int64_t* member_file_off, const snf_bai_carry_t* in, int32_t min_shift, int32_t depth, snf_bai_run_result_t* out) {
  if (!z) { g_berr = "null handle"; return 1; }
  if (min_shift < 8 || min_shift > 30 || depth < 1 || depth > 10 || min_shift + 3 * depth > 40) {
    g_berr = "snf_csi_run: min_shift " + std::to_string(min_shift) + " / depth " + std::to_string(depth) +
             " out of range (min_shift 8..30, depth 1..10, min_shift + 3 depth at most 40)";
    return 1;
  }
  return c_entry(g_berr, z->device, [&] { do_bai_run(z, member_file_off, in, out, true, min_shift, depth); });
}
const char* snf_bai_last_error(void) { return g_berr.c_str(); }
void snf_bgzf_destroy(snf_bgzf_t* z) {
  if (!z) return;
  x_release(z->dev); x_release(z->bai_dev);
  for (hipEvent_t e : z->ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : z->bev) if (e) (void)hipEventDestroy(e);
  delete z;
}
}

// ================================================================================= BGZF deflate: host side ====
struct snf_deflate {
  int device = 0;
  XSlab slab;                    // one grow-only device block carved into the run's arrays
  hipEvent_t ev[2] = {nullptr, nullptr};
  size_t scan_tmp = 0; int64_t scan_n = -1;
  std::vector<uint8_t> h_image; std::vector<int64_t> h_off, h_in_off; std::vector<uint32_t> h_status;
};

namespace {
thread_local std::string g_derr;

void do_deflate_run(snf_deflate* z, const uint8_t* data, int64_t len, const uint32_t* member_len, int64_t n, snf_deflate_result_t* out) {
  if (!out || len < 0 || n < 0 || (len && !data) || (n && !member_len)) snf::fail("snf_deflate_run: null argument");
  if (n >= (1ll << 31) / 2) snf::fail("snf_deflate_run: too many members for one run");
  z->h_in_off.assign((size_t)n + 1, 0);
  int64_t total = 0, bound = 0;
  for (int64_t m = 0; m < n; m++) {
    if (member_len[m] > DZ_MAX) snf::fail("snf_deflate_run: member " + std::to_string(m) + " has " + std::to_string(member_len[m]) + " bytes, a BGZF member takes 65280 (0xff00) at most");
    z->h_in_off[(size_t)m] = total;
    total += member_len[m]; bound += (int64_t)member_len[m] + 31;
  }
  z->h_in_off[(size_t)n] = total;
  if (total != len) snf::fail("snf_deflate_run: the member lengths add up to " + std::to_string((long long)total) + ", the data has " + std::to_string((long long)len) + " bytes");
  const DeflateKnobs k;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(n, k.grid_cap));
  const size_t N1 = (size_t)n + 1;
  if (z->scan_n != n) {
    size_t need = 0;
    SNF_HIP(rocprim::exclusive_scan(nullptr, need, (const uint32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
    z->scan_tmp = need; z->scan_n = n;
  }
  uint8_t *d_in = nullptr, *d_slots = nullptr, *d_image = nullptr; int64_t *d_in_off = nullptr, *d_off = nullptr;
  uint32_t *d_size = nullptr, *d_status = nullptr, *d_tok = nullptr; void* d_tmp = nullptr;
  XSlab& s = z->slab;
  s.measure();
  for (int pass = 0; pass < 2; pass++) {      // measure, then carve
    d_in = s.take<uint8_t>((size_t)len, 32);
    d_in_off = s.take<int64_t>(N1);
    d_slots = s.take<uint8_t>((size_t)n * DZ_SLOT);
    d_size = s.take<uint32_t>(N1);
    d_status = s.take<uint32_t>(N1);
    d_tok = s.take<uint32_t>((size_t)len);
    d_off = s.take<int64_t>(N1);
    d_image = s.take<uint8_t>((size_t)bound, 16);
    d_tmp = s.take<uint8_t>(z->scan_tmp ? z->scan_tmp : 1);
    if (pass == 0) s.reserve();
  }
  x_h2d(d_in, data, (size_t)len);
  x_h2d(d_in_off, z->h_in_off.data(), N1 * 8);
  SNF_HIP(hipMemset(d_size + n, 0, 4));
  for (hipEvent_t& e : z->ev) if (!e) SNF_HIP(hipEventCreate(&e));
  SNF_HIP(hipEventRecord(z->ev[0], 0));
  if (n) {
    const DeflateView v{d_in, d_in_off, d_slots, d_size, d_status, d_tok, (uint32_t)k.max_bits};
    hipLaunchKernelGGL(deflate_member, dim3((unsigned)grid), dim3(DZ_WG), 0, 0, v, n);
    SNF_HIP(hipGetLastError());
  }
  size_t need = z->scan_tmp;
  SNF_HIP(rocprim::exclusive_scan(d_tmp, need, (const uint32_t*)d_size, d_off, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  if (n) {
    const PackView pv{d_slots, d_size, d_off, d_image};
    hipLaunchKernelGGL(deflate_pack, dim3((unsigned)std::min<int64_t>(n, 1 << 16)), dim3(256), 0, 0, pv, n);
    SNF_HIP(hipGetLastError());
  }
  SNF_HIP(hipEventRecord(z->ev[1], 0));
  z->h_off.assign(N1, 0); z->h_status.assign(N1, 0);
  x_d2h(z->h_off.data(), d_off, N1 * 8);
  x_d2h(z->h_status.data(), d_status, (size_t)n * 4);
  for (int64_t m = 0; m < n; m++) if (z->h_status[(size_t)m]) snf::fail("deflate member " + std::to_string(m) + ": the coded size differs from the size the histograms gave");
  const int64_t image_len = z->h_off[(size_t)n];
  if (image_len < 0 || image_len > bound) snf::fail("snf_deflate_run: member sizes out of range");
  z->h_image.resize((size_t)image_len + 1);
  x_d2h(z->h_image.data(), d_image, (size_t)image_len);
  SNF_HIP(hipDeviceSynchronize());
  snf_deflate_result_t r{};
  SNF_HIP(hipEventElapsedTime(&r.ms_kernel, z->ev[0], z->ev[1]));
  r.image = z->h_image.data(); r.image_len = image_len; r.member_off = z->h_off.data(); r.n_members = n;
  *out = r;
}
}  // namespace

extern "C" {
const char* snf_deflate_last_error(void) { return g_derr.c_str(); }
int snf_deflate_create(int device, snf_deflate_t** out) {
  if (!out) { g_derr = "snf_deflate_create: null argument"; return 1; }
  if (c_create(g_derr, device, "deflate")) return 1;
  snf_deflate* z = new snf_deflate();
  z->device = device;
  *out = z;
  return 0;
}
int snf_deflate_run(snf_deflate_t* z, const uint8_t* data, int64_t len, const uint32_t* member_len, int64_t n_members, snf_deflate_result_t* out) {
  if (!z) { g_derr = "null handle"; return 1; }
  return c_entry(g_derr, z->device, [&] { do_deflate_run(z, data, len, member_len, n_members, out); });
}
void snf_deflate_destroy(snf_deflate_t* z) {
  if (!z) return;
  z->slab.release();
  for (hipEvent_t e : z->ev) if (e) (void)hipEventDestroy(e);
  delete z;
}
}

// ============================================================================= reference FASTA in HBM: host side ====
struct snf_fasta {
  int device = 0;
  uint8_t* d_text = nullptr; int64_t cap = 0, len = 0;      // cap + 64 bytes allocated
  std::vector<void*> tmp;                                  // the device arrays of one call
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::vector<int64_t> c_len, c_off, c_lb, c_lw; bool have_index = false;
  std::vector<snf_fasta_record_t> h_rec; std::vector<uint8_t> h_hdr; std::vector<int64_t> h_hdr_off;
  std::vector<int32_t> h_rs, h_re;
  std::vector<uint8_t> h_pool; std::vector<int64_t> h_off; std::vector<int32_t> h_status, h_ncount, h_qs, h_ql;
};

namespace {
thread_local std::string g_ferr;

unsigned fa_grid(int64_t items, const FastaKnobs& k) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(items, k.grid_cap)); }

void fa_events(snf_fasta* f) { for (hipEvent_t& e : f->ev) if (!e) SNF_HIP(hipEventCreate(&e)); }

void fa_room(snf_fasta* f, int64_t more, const char* who = "snf_fasta") {      // (`who`: the handle the buffer serves - snf_vcftext holds one too)
  if (more < 0 || f->len + more > f->cap)
    snf::fail(std::string(who) + ": " + std::to_string((long long)more) + " more bytes behind " + std::to_string((long long)f->len) + " do not fit the " +
              std::to_string((long long)f->cap) + " bytes the handle was created for");
}
void fa_appended(snf_fasta* f, int64_t more) {
  f->len += more;
  SNF_HIP(hipMemset(f->d_text + f->len, 0, 64));
  f->have_index = false;
}

void do_fasta_load_bgzf(snf_fasta* f, const uint8_t* comp, int64_t comp_len, const snf_bgzf_member_t* mem, int64_t n_mem, float* ms, const char* who = "snf_fasta") {
  if (comp_len < 0 || n_mem < 0 || (comp_len && !comp) || (n_mem && !mem)) snf::fail(std::string(who) + "_load_bgzf: null argument");
  int64_t total = 0;
  std::vector<snf_bgzf_member_t> abs((size_t)n_mem);
  for (int64_t m = 0; m < n_mem; m++) {
    const snf_bgzf_member_t& b = mem[m];
    if (b.payload_off < 0 || b.payload_off + (int64_t)b.payload_len > comp_len) snf::fail("BGZF member " + std::to_string(m) + ": payload outside the compressed bytes");
    if (b.isize > BZ_WIN) snf::fail("BGZF member " + std::to_string(m) + ": ISIZE above 65536");
    if (b.out_off != total) snf::fail("BGZF member " + std::to_string(m) + ": out_off is not the exclusive sum of ISIZE");
    abs[(size_t)m] = b; abs[(size_t)m].out_off = f->len + total;      // the kernel writes at text + out_off: the run is appended
    total += b.isize;
  }
  fa_room(f, total, who);
  const BgzfKnobs k;
  x_release(f->tmp);
  uint8_t* d_comp = x_up(f->tmp, comp, (size_t)comp_len, 16);
  snf_bgzf_member_t* d_mem = x_up(f->tmp, abs.data(), (size_t)n_mem);
  uint32_t* d_status = x_alloc<uint32_t>(f->tmp, (size_t)n_mem);
  fa_events(f);
  BgzfView bv{d_comp, d_mem, n_mem, f->d_text, d_status};
  SNF_HIP(hipEventRecord(f->ev[0], 0));
  if (n_mem) {
    if (k.thread_form) hipLaunchKernelGGL(bgzf_inflate_thread, dim3((unsigned)((n_mem + 63) / 64)), dim3(64), 0, 0, bv, n_mem);
    else hipLaunchKernelGGL(bgzf_inflate_wave, dim3((unsigned)std::min<int64_t>(n_mem, k.grid_cap)), dim3(64), 0, 0, bv, n_mem);
    SNF_HIP(hipGetLastError());
  }
  SNF_HIP(hipEventRecord(f->ev[1], 0));
  std::vector<uint32_t> status((size_t)n_mem);
  x_d2h(status.data(), d_status, (size_t)n_mem * 4);
  SNF_HIP(hipDeviceSynchronize());
  x_release(f->tmp);
  for (int64_t m = 0; m < n_mem; m++)
    if (status[(size_t)m]) snf::fail("BGZF member " + std::to_string(m) + ": " + BZ_TEXT[status[(size_t)m] < 8 ? status[(size_t)m] : 4]);
  if (ms) SNF_HIP(hipEventElapsedTime(ms, f->ev[0], f->ev[1]));
  fa_appended(f, total);
}

void do_fasta_index(snf_fasta* f, snf_fasta_index_result_t* out) {
  if (!out) snf::fail("snf_fasta_index: null argument");
  const FastaKnobs k;
  x_release(f->tmp);
  std::vector<void*>& pool = f->tmp;
  const int64_t n = f->len, n_chunks = (n + FA_CHUNK - 1) / FA_CHUNK;
  const size_t N1 = (size_t)n_chunks + 1;
  FaIndexView v{};
  v.text = f->d_text; v.n = n; v.n_chunks = n_chunks;
  v.c_nl = x_alloc<uint32_t>(pool, N1); v.c_cr = x_alloc<uint32_t>(pool, N1); v.c_hdr = x_alloc<uint32_t>(pool, N1);
  int64_t* p_nl = x_alloc<int64_t>(pool, N1); int64_t* p_cr = x_alloc<int64_t>(pool, N1); int64_t* p_hdr = x_alloc<int64_t>(pool, N1);
  v.p_nl = p_nl; v.p_cr = p_cr; v.p_hdr = p_hdr;
  SNF_HIP(hipMemset(v.c_nl + n_chunks, 0, 4)); SNF_HIP(hipMemset(v.c_cr + n_chunks, 0, 4)); SNF_HIP(hipMemset(v.c_hdr + n_chunks, 0, 4));
  size_t need = 0;
  SNF_HIP(rocprim::exclusive_scan(nullptr, need, (const uint32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  void* scan_tmp = x_alloc<uint8_t>(pool, need);
  fa_events(f);
  const unsigned grid = fa_grid(n_chunks, k);
  SNF_HIP(hipEventRecord(f->ev[0], 0));
  if (n_chunks) { hipLaunchKernelGGL(fa_index<false>, dim3(grid), dim3(FA_WG), 0, 0, v); SNF_HIP(hipGetLastError()); }
  SNF_HIP(rocprim::exclusive_scan(scan_tmp, need, (const uint32_t*)v.c_nl, p_nl, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  SNF_HIP(rocprim::exclusive_scan(scan_tmp, need, (const uint32_t*)v.c_cr, p_cr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  SNF_HIP(rocprim::exclusive_scan(scan_tmp, need, (const uint32_t*)v.c_hdr, p_hdr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  int64_t tot_nl = 0, tot_cr = 0, n_rec = 0;
  x_d2h(&tot_nl, p_nl + n_chunks, 8); x_d2h(&tot_cr, p_cr + n_chunks, 8); x_d2h(&n_rec, p_hdr + n_chunks, 8);
  std::vector<FaRec> rec((size_t)n_rec + 1);
  if (n_rec) {
    v.rec = x_alloc<FaRec>(pool, (size_t)n_rec); v.n_rec = n_rec;
    SNF_HIP(hipMemset(v.rec, 0, (size_t)n_rec * sizeof(FaRec)));
    hipLaunchKernelGGL(fa_index<true>, dim3(grid), dim3(FA_WG), 0, 0, v); SNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(fa_lines, dim3(fa_grid(n_rec, k)), dim3(64), 0, 0, v); SNF_HIP(hipGetLastError());
  }
  SNF_HIP(hipEventRecord(f->ev[1], 0));
  x_d2h(rec.data(), v.rec, (size_t)n_rec * sizeof(FaRec));
  // the header lines (names), then the counts of every record's span: what lies between its header line and the next one
  f->h_rec.assign((size_t)n_rec + 1, snf_fasta_record_t{}); f->h_hdr_off.assign((size_t)n_rec + 1, 0);
  int64_t hbytes = 0;
  for (int64_t r = 0; r < n_rec; r++) {
    const FaRec& a = rec[(size_t)r];
    if (a.pos < 0 || a.hdr_end <= a.pos || a.hdr_end > n || a.line_end > n) snf::fail("snf_fasta_index: header table malformed");
    f->h_hdr_off[(size_t)r] = hbytes; hbytes += a.hdr_end - a.pos;
  }
  f->h_hdr_off[(size_t)n_rec] = hbytes;
  f->h_hdr.assign((size_t)hbytes + 1, 0);
  for (int64_t r = 0; r < n_rec; r++) x_d2h(f->h_hdr.data() + f->h_hdr_off[(size_t)r], f->d_text + rec[(size_t)r].pos, (size_t)(rec[(size_t)r].hdr_end - rec[(size_t)r].pos));
  for (int64_t r = 0; r < n_rec; r++) {
    const FaRec& a = rec[(size_t)r];
    const bool last = r + 1 == n_rec;
    const int64_t nl_next = last ? tot_nl : rec[(size_t)r + 1].nl_before, cr_next = last ? tot_cr : rec[(size_t)r + 1].cr_before;
    const bool hdr_nl = a.hdr_end < n, hdr_cr = f->h_hdr[(size_t)(f->h_hdr_off[(size_t)r + 1] - 1)] == 13;
    snf_fasta_record_t& o = f->h_rec[(size_t)r];
    o.header_start = a.pos; o.header_end = a.hdr_end; o.line_start = a.hdr_end + 1; o.line_end = a.line_end; o.line_cr = (int32_t)a.line_cr;
    o.span_end = last ? n : rec[(size_t)r + 1].pos;
    o.n_newline = nl_next - a.nl_before - (hdr_nl ? 1 : 0); o.n_cr = cr_next - a.cr_before - (hdr_cr ? 1 : 0);
  }
  SNF_HIP(hipDeviceSynchronize());
  snf_fasta_index_result_t r{};
  SNF_HIP(hipEventElapsedTime(&r.ms_kernel, f->ev[0], f->ev[1]));
  r.n_records = n_rec; r.rec = f->h_rec.data(); r.headers = f->h_hdr.data(); r.header_off = f->h_hdr_off.data(); r.text_len = n;
  x_release(pool);
  *out = r;
}

void do_fasta_set_index(snf_fasta* f, int64_t n, const int64_t* length, const int64_t* offset, const int64_t* lb, const int64_t* lw) {
  if (n < 0 || (n && (!length || !offset || !lb || !lw))) snf::fail("snf_fasta_set_index: null argument");
  for (int64_t c = 0; c < n; c++) {
    const std::string at = "snf_fasta_set_index: contig " + std::to_string((long long)c);
    if (length[c] < 0 || length[c] >= (1ll << 31)) snf::fail(at + " has " + std::to_string((long long)length[c]) + " bases, base coordinates are 32-bit");
    if (lb[c] < 1 || lw[c] < lb[c] || lw[c] >= (1ll << 31)) snf::fail(at + ": line of " + std::to_string((long long)lb[c]) + " bases in " + std::to_string((long long)lw[c]) + " bytes");
    if (offset[c] < 0) snf::fail(at + ": negative offset");
    if (length[c]) {
      const int64_t lastb = offset[c] + ((length[c] - 1) / lb[c]) * lw[c] + (length[c] - 1) % lb[c];
      if (lastb >= f->len) snf::fail(at + ": its last base lies at byte " + std::to_string((long long)lastb) + ", the text has " + std::to_string((long long)f->len) + " bytes (an index of another file?)");
    }
  }
  f->c_len.assign(length, length + n); f->c_off.assign(offset, offset + n); f->c_lb.assign(lb, lb + n); f->c_lw.assign(lw, lw + n);
  f->have_index = true;
}

void fa_contig(snf_fasta* f, int64_t contig, const char* who) {
  if (!f->have_index) snf::fail(std::string(who) + " before snf_fasta_set_index");
  if (contig < 0 || contig >= (int64_t)f->c_len.size()) snf::fail(std::string(who) + ": contig index out of range");
}

void do_fasta_nruns(snf_fasta* f, int64_t contig, int32_t lo, int32_t hi, snf_fasta_runs_t* out) {
  if (!out) snf::fail("snf_fasta_nruns: null argument");
  fa_contig(f, contig, "snf_fasta_nruns");
  const int64_t length = f->c_len[(size_t)contig], offset = f->c_off[(size_t)contig], lb = f->c_lb[(size_t)contig], lw = f->c_lw[(size_t)contig];
  if (lo < 0 || hi < lo || hi > length) snf::fail("snf_fasta_nruns: [" + std::to_string(lo) + ", " + std::to_string(hi) + ") is not a clipped range of a contig of " + std::to_string((long long)length) + " bases");
  snf_fasta_runs_t r{};
  f->h_rs.assign(1, 0); f->h_re.assign(1, 0);
  r.start = f->h_rs.data(); r.end = f->h_re.data(); r.regular = 1;
  if (hi == lo) { *out = r; return; }
  const FastaKnobs k;
  x_release(f->tmp);
  std::vector<void*>& pool = f->tmp;
  FaRunsView v{};
  v.text = f->d_text; v.lo = lo;
  v.b0 = offset + (lo / lb) * lw + lo % lb; v.b1 = offset + ((hi - 1) / lb) * lw + (hi - 1) % lb + 1;      // < f->len: checked by set_index
  v.a0 = v.b0 & ~(int64_t)(FA_VEC - 1);
  v.n_chunks = (v.b1 - v.a0 + FA_CHUNK - 1) / FA_CHUNK;
  const size_t N1 = (size_t)v.n_chunks + 1;
  v.c_se = x_alloc<unsigned long long>(pool, N1); v.c_le = x_alloc<uint32_t>(pool, N1);
  unsigned long long* p_se = x_alloc<unsigned long long>(pool, N1); int64_t* p_le = x_alloc<int64_t>(pool, N1);
  v.p_se = p_se; v.p_le = p_le;
  SNF_HIP(hipMemset(v.c_se + v.n_chunks, 0, 8)); SNF_HIP(hipMemset(v.c_le + v.n_chunks, 0, 4));
  size_t need_a = 0, need_b = 0;
  SNF_HIP(rocprim::exclusive_scan(nullptr, need_a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, N1, rocprim::plus<unsigned long long>(), 0));
  SNF_HIP(rocprim::exclusive_scan(nullptr, need_b, (const uint32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  void* tmp_a = x_alloc<uint8_t>(pool, need_a); void* tmp_b = x_alloc<uint8_t>(pool, need_b);
  fa_events(f);
  const unsigned grid = fa_grid(v.n_chunks, k);
  SNF_HIP(hipEventRecord(f->ev[0], 0));
  hipLaunchKernelGGL(fa_nruns<false>, dim3(grid), dim3(FA_WG), 0, 0, v); SNF_HIP(hipGetLastError());
  SNF_HIP(rocprim::exclusive_scan(tmp_a, need_a, (const unsigned long long*)v.c_se, p_se, 0ull, N1, rocprim::plus<unsigned long long>(), 0));
  SNF_HIP(rocprim::exclusive_scan(tmp_b, need_b, (const uint32_t*)v.c_le, p_le, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  unsigned long long tot_se = 0; int64_t tot_le = 0;
  x_d2h(&tot_se, p_se + v.n_chunks, 8); x_d2h(&tot_le, p_le + v.n_chunks, 8);
  const int64_t n_runs = (int64_t)(tot_se & 0xffffffffull);
  if ((int64_t)(tot_se >> 32) != n_runs) snf::fail("snf_fasta_nruns: opens and closes differ");
  r.regular = (v.b1 - v.b0) - tot_le == (int64_t)hi - lo ? 1 : 0;      // else: lines of another width than the index says - the runs are not returned
  if (n_runs && r.regular) {
    v.start = x_alloc<int32_t>(pool, (size_t)n_runs); v.end = x_alloc<int32_t>(pool, (size_t)n_runs); v.n_runs = n_runs;
    hipLaunchKernelGGL(fa_nruns<true>, dim3(grid), dim3(FA_WG), 0, 0, v); SNF_HIP(hipGetLastError());
  }
  SNF_HIP(hipEventRecord(f->ev[1], 0));
  if (n_runs && r.regular) {
    f->h_rs.assign((size_t)n_runs, 0); f->h_re.assign((size_t)n_runs, 0);
    x_d2h(f->h_rs.data(), v.start, (size_t)n_runs * 4); x_d2h(f->h_re.data(), v.end, (size_t)n_runs * 4);
    r.n_runs = n_runs; r.start = f->h_rs.data(); r.end = f->h_re.data();
  }
  SNF_HIP(hipDeviceSynchronize());
  SNF_HIP(hipEventElapsedTime(&r.ms_kernel, f->ev[0], f->ev[1]));
  x_release(pool);
  *out = r;
}

void do_fasta_fetch(snf_fasta* f, int64_t contig, int64_t n, const int64_t* start, const int64_t* end, snf_fasta_fetch_t* out) {
  if (!out || n < 0 || (n && (!start || !end))) snf::fail("snf_fasta_fetch: null argument");
  if (!f->have_index) snf::fail("snf_fasta_fetch before snf_fasta_set_index");
  if (contig >= (int64_t)f->c_len.size()) snf::fail("snf_fasta_fetch: contig index out of range");
  const bool known = contig >= 0;
  const int64_t length = known ? f->c_len[(size_t)contig] : 0;
  f->h_off.assign((size_t)n + 1, 0); f->h_status.assign((size_t)n + 1, 0); f->h_ncount.assign((size_t)n + 1, 0);
  f->h_qs.assign((size_t)n + 1, 0); f->h_ql.assign((size_t)n + 1, 0);
  int64_t total = 0;
  for (int64_t q = 0; q < n; q++) {      // FastaFile.fetch, statement for statement
    int32_t st = SNF_FASTA_OK; int64_t len = 0;
    const int64_t s = start[q], e = std::min(end[q], length);
    if (!known) st = SNF_FASTA_KEY_ERROR;
    else if (s < 0) st = SNF_FASTA_START_NEGATIVE;
    else if (s > e) { if (s < length) st = SNF_FASTA_START_ABOVE_END; }
    else len = e - s;
    f->h_status[(size_t)q] = st; f->h_off[(size_t)q] = total; f->h_qs[(size_t)q] = (int32_t)(len ? s : 0); f->h_ql[(size_t)q] = (int32_t)len;
    total += len;
  }
  f->h_off[(size_t)n] = total;
  f->h_pool.assign((size_t)total + 1, 0);
  snf_fasta_fetch_t r{};
  if (total) {
    const FastaKnobs k;
    x_release(f->tmp);
    std::vector<void*>& pool = f->tmp;
    FaGatherView v{};
    v.text = f->d_text; v.offset = f->c_off[(size_t)contig]; v.lb = (uint32_t)f->c_lb[(size_t)contig]; v.lw = (uint32_t)f->c_lw[(size_t)contig];
    v.start = x_up(pool, f->h_qs.data(), (size_t)n); v.len = x_up(pool, f->h_ql.data(), (size_t)n); v.off = x_up(pool, f->h_off.data(), (size_t)n + 1);
    v.pool = x_alloc<uint8_t>(pool, (size_t)total); v.n_count = x_alloc<int32_t>(pool, (size_t)n);
    fa_events(f);
    SNF_HIP(hipEventRecord(f->ev[0], 0));
    hipLaunchKernelGGL(fa_gather, dim3(fa_grid(n, k)), dim3(64), 0, 0, v, n); SNF_HIP(hipGetLastError());
    SNF_HIP(hipEventRecord(f->ev[1], 0));
    x_d2h(f->h_pool.data(), v.pool, (size_t)total); x_d2h(f->h_ncount.data(), v.n_count, (size_t)n * 4);
    SNF_HIP(hipDeviceSynchronize());
    SNF_HIP(hipEventElapsedTime(&r.ms_kernel, f->ev[0], f->ev[1]));
    x_release(pool);
  }
  r.n = n; r.pool = f->h_pool.data(); r.off = f->h_off.data(); r.status = f->h_status.data(); r.n_count = f->h_ncount.data();
  *out = r;
}
}  // namespace

template <class F> static int fa_entry(snf_fasta* f, F&& body) {
  if (!f) { g_ferr = "null handle"; return 1; }
  return c_entry(g_ferr, f->device, body);
}

extern "C" {
const char* snf_fasta_last_error(void) { return g_ferr.c_str(); }
int snf_fasta_create(int device, int64_t capacity, snf_fasta_t** out) {
  if (!out || capacity < 0) { g_ferr = "snf_fasta_create: null argument"; return 1; }
  if (c_create(g_ferr, device, "FASTA")) return 1;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)capacity + 64) != hipSuccess) {
    (void)hipGetLastError();
    g_ferr = "reference of " + std::to_string((long long)capacity) + " bytes does not fit device " + std::to_string(device);
    return 1;
  }
  if (hipMemset(p, 0, (size_t)capacity + 64) != hipSuccess) { (void)hipFree(p); g_ferr = "hipMemset failed"; return 1; }
  snf_fasta* f = new snf_fasta();
  f->device = device; f->d_text = (uint8_t*)p; f->cap = capacity;
  *out = f;
  return 0;
}
int snf_fasta_load_text(snf_fasta_t* f, const uint8_t* bytes, int64_t len) {
  return fa_entry(f, [&] { if (len < 0 || (len && !bytes)) snf::fail("snf_fasta_load_text: null argument"); fa_room(f, len); x_h2d(f->d_text + f->len, bytes, (size_t)len); fa_appended(f, len); });
}
int snf_fasta_load_bgzf(snf_fasta_t* f, const uint8_t* compressed, int64_t compressed_len, const snf_bgzf_member_t* members, int64_t n_members, float* ms_inflate) {
  return fa_entry(f, [&] { do_fasta_load_bgzf(f, compressed, compressed_len, members, n_members, ms_inflate); });
}
int snf_fasta_index(snf_fasta_t* f, snf_fasta_index_result_t* out) { return fa_entry(f, [&] { do_fasta_index(f, out); }); }
int snf_fasta_set_index(snf_fasta_t* f, int64_t n_contigs, const int64_t* length, const int64_t* offset, const int64_t* line_bases, const int64_t* line_width) {
  return fa_entry(f, [&] { do_fasta_set_index(f, n_contigs, length, offset, line_bases, line_width); });
}
int snf_fasta_nruns(snf_fasta_t* f, int64_t contig, int32_t lo, int32_t hi, snf_fasta_runs_t* out) { return fa_entry(f, [&] { do_fasta_nruns(f, contig, lo, hi, out); }); }
int snf_fasta_fetch(snf_fasta_t* f, int64_t contig, int64_t n, const int64_t* start, const int64_t* end, snf_fasta_fetch_t* out) {
  return fa_entry(f, [&] { do_fasta_fetch(f, contig, n, start, end, out); });
}
int snf_fasta_read_text(snf_fasta_t* f, int64_t off, int64_t len, uint8_t* dst) {
  return fa_entry(f, [&] { if (len && !dst) snf::fail("snf_fasta_read_text: null argument");
                           if (off < 0 || len < 0 || off + len > f->len) snf::fail("snf_fasta_read_text: range outside the text");
                           x_d2h(dst, f->d_text + off, (size_t)len); });
}
void snf_fasta_destroy(snf_fasta_t* f) {
  if (!f) return;
  x_release(f->tmp);
  if (f->d_text) (void)hipFree(f->d_text);
  for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
  delete f;
}
}

// ================================================================================ target VCF in HBM: host side ====
struct snf_vcftext {
  snf_fasta fa;                                            // the text buffer and its loaders are the FASTA's (do_fasta_load_bgzf appends into it)
  snf_vcftext_line_t* d_line = nullptr; int64_t n_lines = -1;      // the line table stays resident for the rewrite
  std::vector<snf_vcftext_line_t> h_line;
  std::vector<uint8_t> h_pool; std::vector<int64_t> h_off;
};

namespace {
thread_local std::string g_verr;

unsigned vt_grid(int64_t items, int32_t max_grid) {
  const int64_t cap = max_grid > 0 ? max_grid : (1 << 20);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(items, cap));
}

void vt_drop_table(snf_vcftext* t) {
  if (t->d_line) { x_free(t->d_line); t->d_line = nullptr; }
  t->n_lines = -1;
}

void do_vcftext_parse(snf_vcftext* t, int32_t max_grid, snf_vcftext_table_t* out) {
  if (!out) snf::fail("snf_vcftext_parse: null argument");
  snf_fasta* f = &t->fa;
  vt_drop_table(t);
  x_release(f->tmp);
  std::vector<void*>& pool = f->tmp;
  const int64_t n = f->len, n_chunks = (n + VT_CHUNK - 1) / VT_CHUNK;
  const size_t N1 = (size_t)n_chunks + 1;
  VtLinesView lv{};
  lv.text = f->d_text; lv.n = n; lv.n_chunks = n_chunks;
  lv.c_ls = x_alloc<uint32_t>(pool, N1);
  int64_t* p_ls = x_alloc<int64_t>(pool, N1);
  lv.p_ls = p_ls;
  SNF_HIP(hipMemset(lv.c_ls + n_chunks, 0, 4));
  size_t need = 0;
  SNF_HIP(rocprim::exclusive_scan(nullptr, need, (const uint32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  void* scan_tmp = x_alloc<uint8_t>(pool, need);
  fa_events(f);
  hipEvent_t ev2 = nullptr;
  SNF_HIP(hipEventCreate(&ev2));
  snf_vcftext_table_t r{};
  try {
    const unsigned grid = vt_grid(n_chunks, max_grid);
    SNF_HIP(hipEventRecord(f->ev[0], 0));
    if (n_chunks) { hipLaunchKernelGGL(vt_lines<false>, dim3(grid), dim3(VT_WG), 0, 0, lv); SNF_HIP(hipGetLastError()); }
    SNF_HIP(rocprim::exclusive_scan(scan_tmp, need, (const uint32_t*)lv.c_ls, p_ls, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
    int64_t n_lines = 0;
    x_d2h(&n_lines, p_ls + n_chunks, 8);
    if (n_lines < 0 || n_lines > n) snf::fail("snf_vcftext_parse: line count out of range");
    lv.line_start = x_alloc<int64_t>(pool, (size_t)n_lines + 1); lv.n_lines = n_lines;
    x_h2d(lv.line_start + n_lines, &n, 8);
    if (n_lines) { hipLaunchKernelGGL(vt_lines<true>, dim3(grid), dim3(VT_WG), 0, 0, lv); SNF_HIP(hipGetLastError()); }
    SNF_HIP(hipEventRecord(f->ev[1], 0));
    void* dl = nullptr;
    const size_t lbytes = ((size_t)n_lines + 1) * sizeof(snf_vcftext_line_t);
    if (hipMalloc(&dl, lbytes) != hipSuccess) {
      (void)hipGetLastError();
      snf::fail("line table of " + std::to_string(lbytes) + " bytes does not fit device " + std::to_string(f->device));
    }
    t->d_line = (snf_vcftext_line_t*)dl;
    VtParseView pv{f->d_text, n, lv.line_start, t->d_line, n_lines};
    if (n_lines) {
      hipLaunchKernelGGL(vt_parse, dim3(vt_grid(n_lines, max_grid)), dim3(64), 0, 0, pv); SNF_HIP(hipGetLastError());
      hipLaunchKernelGGL(vt_chrom, dim3(vt_grid((n_lines + VT_CHROM_WG - 1) / VT_CHROM_WG, max_grid)), dim3(VT_CHROM_WG), 0, 0, pv); SNF_HIP(hipGetLastError());
    }
    SNF_HIP(hipEventRecord(ev2, 0));
    t->h_line.assign((size_t)n_lines + 1, snf_vcftext_line_t{});
    x_d2h(t->h_line.data(), t->d_line, (size_t)n_lines * sizeof(snf_vcftext_line_t));
    SNF_HIP(hipDeviceSynchronize());
    SNF_HIP(hipEventElapsedTime(&r.ms_lines, f->ev[0], f->ev[1]));
    SNF_HIP(hipEventElapsedTime(&r.ms_parse, f->ev[1], ev2));
    t->n_lines = n_lines;
    r.n_lines = n_lines; r.text_len = n; r.line = t->h_line.data();
  } catch (...) {
    (void)hipEventDestroy(ev2);
    x_release(pool);
    vt_drop_table(t);
    throw;
  }
  (void)hipEventDestroy(ev2);
  x_release(pool);
  *out = r;
}

// the scan over the row sizes, the copy and the way back - what gather and rewrite share
template <bool REWRITE>
void vt_rows_out(snf_vcftext* t, VtCopyView v, int32_t max_grid, snf_vcftext_pool_t* out) {
  snf_fasta* f = &t->fa;
  std::vector<void*>& pool = f->tmp;
  const int64_t n = v.n;
  const size_t N1 = (size_t)n + 1;
  v.size = x_alloc<int64_t>(pool, N1);
  int64_t* d_off = x_alloc<int64_t>(pool, N1);
  SNF_HIP(hipMemset(v.size + n, 0, 8));
  size_t need = 0;
  SNF_HIP(rocprim::exclusive_scan(nullptr, need, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  void* scan_tmp = x_alloc<uint8_t>(pool, need);
  fa_events(f);
  SNF_HIP(hipEventRecord(f->ev[0], 0));
  if (n) { hipLaunchKernelGGL(vt_size<REWRITE>, dim3(vt_grid((n + VT_CHROM_WG - 1) / VT_CHROM_WG, max_grid)), dim3(VT_CHROM_WG), 0, 0, v); SNF_HIP(hipGetLastError()); }
  SNF_HIP(rocprim::exclusive_scan(scan_tmp, need, (const int64_t*)v.size, d_off, (int64_t)0, N1, rocprim::plus<int64_t>(), 0));
  t->h_off.assign(N1, 0);
  x_d2h(t->h_off.data(), d_off, N1 * 8);
  const int64_t total = t->h_off[(size_t)n];
  if (total < 0) snf::fail("snf_vcftext: row sizes out of range");
  v.out_off = d_off; v.out = x_alloc<uint8_t>(pool, (size_t)total, 16);
  if (n && total) { hipLaunchKernelGGL(vt_copy<REWRITE>, dim3(vt_grid(n, max_grid)), dim3(64), 0, 0, v); SNF_HIP(hipGetLastError()); }
  SNF_HIP(hipEventRecord(f->ev[1], 0));
  t->h_pool.resize((size_t)total + 1);
  x_d2h(t->h_pool.data(), v.out, (size_t)total);
  SNF_HIP(hipDeviceSynchronize());
  snf_vcftext_pool_t r{};
  SNF_HIP(hipEventElapsedTime(&r.ms_kernel, f->ev[0], f->ev[1]));
  r.n = n; r.pool = t->h_pool.data(); r.off = t->h_off.data();
  x_release(pool);
  *out = r;
}

void do_vcftext_gather(snf_vcftext* t, int64_t n, const int64_t* off, const int64_t* len, int32_t max_grid, snf_vcftext_pool_t* out) {
  if (!out || n < 0 || (n && (!off || !len))) snf::fail("snf_vcftext_gather: null argument");
  snf_fasta* f = &t->fa;
  for (int64_t r = 0; r < n; r++)
    if (off[r] < 0 || len[r] < 0 || off[r] > f->len || len[r] > f->len - off[r]) snf::fail("snf_vcftext_gather: span " + std::to_string((long long)r) + " outside the text");
  x_release(f->tmp);
  VtCopyView v{};
  v.text = f->d_text; v.n = n;
  v.row_off = x_up(f->tmp, off, (size_t)n); v.row_len = x_up(f->tmp, len, (size_t)n);
  try { vt_rows_out<false>(t, v, max_grid, out); } catch (...) { x_release(f->tmp); throw; }
}

void do_vcftext_rewrite(snf_vcftext* t, int64_t n, const int64_t* line, const int32_t* sid, int64_t n_suffix, const uint8_t* spool, const int64_t* soff,
                        int32_t max_grid, snf_vcftext_pool_t* out) {
  if (!out || n < 0 || n_suffix < 0 || (n && (!line || !sid)) || !soff) snf::fail("snf_vcftext_rewrite: null argument");
  if (t->n_lines < 0) snf::fail("snf_vcftext_rewrite before a successful snf_vcftext_parse");
  if (soff[0] != 0) snf::fail("snf_vcftext_rewrite: suffix_off[0] is not 0");
  for (int64_t s = 0; s < n_suffix; s++) if (soff[s + 1] < soff[s]) snf::fail("snf_vcftext_rewrite: suffix_off decreases");
  if (soff[n_suffix] && !spool) snf::fail("snf_vcftext_rewrite: null argument");
  for (int64_t r = 0; r < n; r++) {
    if (line[r] < -1 || line[r] >= t->n_lines) snf::fail("snf_vcftext_rewrite: row " + std::to_string((long long)r) + ": no such line");
    if (line[r] < 0) continue;
    if (t->h_line[(size_t)line[r]].cls != SNF_VT_RECORD) snf::fail("snf_vcftext_rewrite: row " + std::to_string((long long)r) + ": line " + std::to_string((long long)line[r] + 1) + " was not parsed on the device");
    if (sid[r] < 0 || sid[r] >= n_suffix) snf::fail("snf_vcftext_rewrite: row " + std::to_string((long long)r) + ": no such suffix");
  }
  snf_fasta* f = &t->fa;
  x_release(f->tmp);
  VtCopyView v{};
  v.text = f->d_text; v.n = n; v.line = t->d_line; v.n_lines = t->n_lines;
  v.row_line = x_up(f->tmp, line, (size_t)n); v.row_suffix = x_up(f->tmp, sid, (size_t)n);
  v.suffix = x_up(f->tmp, spool, (size_t)soff[n_suffix]); v.suffix_off = x_up(f->tmp, soff, (size_t)n_suffix + 1);
  try { vt_rows_out<true>(t, v, max_grid, out); } catch (...) { x_release(f->tmp); throw; }
}
}  // namespace

template <class F> static int vt_entry(snf_vcftext* t, F&& body) {
  if (!t) { g_verr = "null handle"; return 1; }
  return c_entry(g_verr, t->fa.device, body);
}

extern "C" {
const char* snf_vcftext_last_error(void) { return g_verr.c_str(); }
int snf_vcftext_create(int device, int64_t capacity, snf_vcftext_t** out) {
  if (!out || capacity < 0) { g_verr = "snf_vcftext_create: null argument"; return 1; }
  if (c_create(g_verr, device, "target-text")) return 1;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)capacity + 64) != hipSuccess) {
    (void)hipGetLastError();
    g_verr = "target VCF of " + std::to_string((long long)capacity) + " bytes does not fit device " + std::to_string(device);
    return 1;
  }
  if (hipMemset(p, 0, (size_t)capacity + 64) != hipSuccess) { (void)hipFree(p); g_verr = "hipMemset failed"; return 1; }
  snf_vcftext* t = new snf_vcftext();
  t->fa.device = device; t->fa.d_text = (uint8_t*)p; t->fa.cap = capacity;
  *out = t;
  return 0;
}
int snf_vcftext_load_text(snf_vcftext_t* t, const uint8_t* bytes, int64_t len) {
  return vt_entry(t, [&] { if (len < 0 || (len && !bytes)) snf::fail("snf_vcftext_load_text: null argument");
                           vt_drop_table(t); fa_room(&t->fa, len, "snf_vcftext"); x_h2d(t->fa.d_text + t->fa.len, bytes, (size_t)len); fa_appended(&t->fa, len); });
}
int snf_vcftext_load_bgzf(snf_vcftext_t* t, const uint8_t* compressed, int64_t compressed_len, const snf_bgzf_member_t* members, int64_t n_members, float* ms_inflate) {
  return vt_entry(t, [&] { vt_drop_table(t); do_fasta_load_bgzf(&t->fa, compressed, compressed_len, members, n_members, ms_inflate, "snf_vcftext"); });
}
int snf_vcftext_parse(snf_vcftext_t* t, int32_t max_grid, snf_vcftext_table_t* out) { return vt_entry(t, [&] { do_vcftext_parse(t, max_grid, out); }); }
int snf_vcftext_gather(snf_vcftext_t* t, int64_t n, const int64_t* off, const int64_t* len, int32_t max_grid, snf_vcftext_pool_t* out) {
  return vt_entry(t, [&] { do_vcftext_gather(t, n, off, len, max_grid, out); });
}
int snf_vcftext_rewrite(snf_vcftext_t* t, int64_t n_rows, const int64_t* line, const int32_t* suffix_id, int64_t n_suffix, const uint8_t* suffix_pool,
                        const int64_t* suffix_off, int32_t max_grid, snf_vcftext_pool_t* out) {
  return vt_entry(t, [&] { do_vcftext_rewrite(t, n_rows, line, suffix_id, n_suffix, suffix_pool, suffix_off, max_grid, out); });
}
void snf_vcftext_destroy(snf_vcftext_t* t) {
  if (!t) return;
  vt_drop_table(t);
  x_release(t->fa.tmp);
  if (t->fa.d_text) (void)hipFree(t->fa.d_text);
  for (hipEvent_t e : t->fa.ev) if (e) (void)hipEventDestroy(e);
  delete t;
}
}
