// snf_knobs.h - every SNF_* environment switch of the HIP library, read here and nowhere else (host code only; plain C++, it
// builds under g++ for the GPU-less test tier).  README.md holds the same list as a table; tests/test_knobs.py keeps the two equal.
//
// WHEN a switch is read is part of the contract (include/sniffles_amd.h):
//   BatchKnobs    constructing one reads the environment.  snf_batch_impl holds one as a const member, so a handle's switches are
//                 those of the environment at snf_batch_create and hold until snf_batch_destroy: upload, every pass, every fetch
//                 read b->k.<field>, never the environment.  A switch whose default depends on the data keeps an "unset" value (-1 or
//                 KNOB_UNSET)
//                 here and is resolved where the data is known.
//   ProcessKnobs  what configures state shared by all handles of the process (pacing, pools, arenas): once per process, at the
//                 first use of process_knobs().
//   ExtractKnobs / BgzfKnobs / BaiKnobs / DeflateKnobs / FastaKnobs / CombineKnobs   the entry points without a long-lived handle: constructed at the top of each call.
// The parses are not uniform on purpose - each keeps the meaning its switch always had ("set at all", "atoi != 0", clamped, a
// string compared).  Defaults are the product path; everything else exists for tests and measurements.
#pragma once
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

namespace snf {

constexpr int KNOB_UNSET = INT_MIN;   // a switch whose "not set" differs from every value it can be set to
inline bool env_set(const char* name) { return getenv(name) != nullptr; }                                   // set at all, even to "0" or ""
inline int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
inline int env_pos(const char* name, int other) { const int v = env_int(name, 0); return v > 0 ? v : other; }   // set and > 0, else `other`
inline bool env_on(const char* name) { return env_int(name, 0) != 0; }                                      // set and atoi != 0
inline bool env_is(const char* name, const char* value) { const char* e = getenv(name); return e && strcmp(e, value) == 0; }
inline std::string env_str(const char* name) { const char* e = getenv(name); return e ? e : ""; }

struct BatchKnobs {
  // ---- which form of the pass
  bool wave_path = !env_set("SNF_NO_WAVE");          // SNF_NO_WAVE (set at all): thread-per-item kernels only; default: the wave kernels
  bool fuse = !env_set("SNF_NO_FUSE");               // SNF_NO_FUSE (set): rocPRIM scans instead of the fused flag / scan / emit pairs (snf_fused.h);
                                                     //   also: no window front end, no deferred read names
  bool sort64 = env_set("SNF_SORT64");               // SNF_SORT64 (set): tests - force the wide-key sorts; default: 32-bit keys where they fit
  bool prefilter = !env_set("SNF_NO_PREFILTER");     // SNF_NO_PREFILTER (set): every lead through the sort; default: the occupancy prefilter
  bool winfront = !env_set("SNF_NO_WINFRONT");       // SNF_NO_WINFRONT (set): the sort path instead of the window front end (snf_stage_window.h)
  int win_bits = env_int("SNF_WIN_BITS", 0);         // SNF_WIN_BITS=k: window width forced to 2^k bins (6..win_bits_max; 0 / out of range: chosen from the data)
  int win_bits_max = [] { const int v = env_int("SNF_WIN_BITS_MAX", 10); return v >= 6 && v <= 12 ? v : 10; }();   // SNF_WIN_BITS_MAX=6..12, default 10 (anything
                                                     //   else: 10): widest window tried (measured on the 30x genome: 10 beats 9 and 8).  12 is what win_pack's bin field
                                                     //   holds (snf_stage_window.h), 6 the narrowest window do_upload sizes its arrays for (WIN_W_MIN)
  bool w4_split = env_on("SNF_W4_SPLIT");            // SNF_W4_SPLIT!=0: w4s_segment as its small instance + the large one over a list; default: one launch
  bool pool_slices = !env_set("SNF_NO_POOL_SLICES"); // SNF_NO_POOL_SLICES (set): fused sequences through the shared counter only; default: a private slice per resident wave
  int fuse_copy = env_set("SNF_FUSE_COPY") ? env_on("SNF_FUSE_COPY") : -1;   // SNF_FUSE_COPY=0/1: the parts of fused sequences copied inside the refine kernels / by d1c_fusecopy
                                                     //   on the side stream; unset (-1): the side stream for handles whose passes are eager, in place for those that replay a graph
  bool merge_reread = env_on("SNF_MERGE_REREAD");    // SNF_MERGE_REREAD!=0: merged cluster metrics read again instead of added (tests/test_clusters.py)
  int run_gap = env_int("SNF_RUN_GAP", KNOB_UNSET);  // SNF_RUN_GAP=<bp>: cut width of the parallel merge scan (negative: whole group serial);
                                                     //   unset: max(1000, cluster_merge_bnd, cluster_repeat_h_max) - resolved at create
  int chain = env_set("SNF_CHAIN") ? env_on("SNF_CHAIN") : env_set("SNF_NO_CHAIN") ? 0 : -1;   // SNF_CHAIN=0/1 (SNF_NO_CHAIN set = 0): scan chains as launch pairs /
                                                     //   single launches; unset (-1): on for batches of <= 400 k leads (resolved at upload)
  int graph = env_set("SNF_GRAPH") ? env_on("SNF_GRAPH") : env_set("SNF_NO_GRAPH") ? 0 : -1;   // SNF_GRAPH=0/1 (SNF_NO_GRAPH set = 0): passes eager / replayed from
                                                     //   a HIP graph; unset (-1): as SNF_CHAIN
  int heavy_n = env_int("SNF_HEAVY_N", 24);          // SNF_HEAVY_N=n, default 24: hand-over lists put items above n leads at the front (9..63; 0 / out of range: one class)
  int e1_batch = env_int("SNF_E1_BATCH", 64);        // SNF_E1_BATCH=k, default 64: calls per wave of the finalize kernel (2, 4, 8, 16, 32; anything else: 64)
  bool big_stage = !env_set("SNF_NO_BIG_STAGE");     // SNF_NO_BIG_STAGE (set): no LDS staging in the big-cluster kernels; default x_big<0>: clusters up to
                                                     //   SNF_BIG_STAGE_CAP leads are kept in LDS
  bool cov_exact = env_set("SNF_COV_EXACT");         // SNF_COV_EXACT (set): the exact coverage walk (snf_cov.h) for every task; default: masked / wrapping tasks only
  bool d4_thread = env_is("SNF_D4", "thread");       // SNF_D4=thread: coverage samples by the former thread-per-call kernel d4_coverage; default d4s_coverage
  bool d1_groups = !env_set("SNF_NO_D1_GROUPS");     // SNF_NO_D1_GROUPS (set): a wave per merged cluster in merge_inner / resplit; default: small ones eight per wave (snf_wave_refine_g.h)
  bool d2_groups = !env_set("SNF_NO_D2_GROUPS");     // SNF_NO_D2_GROUPS (set): a wave per refined cluster in call_from; default: small ones several per wave (snf_wave_call_g.h)
  bool d2_mid = env_set("SNF_D2_MID");               // SNF_D2_MID (set): A/B - clusters of 9..32 leads two per wave (measured slower than a wave each)
  bool rn_defer = !env_set("SNF_NO_RN_DEFER");       // SNF_NO_RN_DEFER (set): all read names in the candidate stage; default (SNF_OUT_EXECUTE): only for the calls that pass QC
  bool rn_fuse = !env_set("SNF_NO_RN_FUSE");         // SNF_NO_RN_FUSE (set): read names of the kept calls by a pass of their own; default: written by f4w_emit
  // ---- grids, occupancy, scheduling inside a pass (experiments)
  int cons_nw = env_int("SNF_CONS_NW", 1);           // SNF_CONS_NW=1/4: waves per SMALL consensus call; 1 (default): single-wave workgroups leave room for the LARGE class next
                                                     //   to them - LARGE in place 0.75 -> 0.5 ms, the pass 2.5 % shorter
  int cons_large_nw = env_int("SNF_CONS_LARGE_NW", 4); // SNF_CONS_LARGE_NW=4/8/16, default 4: waves per LARGE consensus call
  int cons_order = env_int("SNF_CONS_ORDER", -1);    // SNF_CONS_ORDER=0/1/2: order of the consensus classes (enqueue_consensus_wave); unset (< 0): 2 with another pass in flight, else 0
  bool serial = env_set("SNF_SERIAL");               // SNF_SERIAL (set): dev - every ALT kernel alone on the device (isolated timings); no pass graph
  bool readprep_each_pass = env_set("SNF_READPREP_EACH_PASS");   // SNF_READPREP_EACH_PASS (set): BOTH indexes built at upload - the read index and the window index (w1_hist .. w3_scatter) -
                                                                 // are rebuilt in every call_candidates instead (the read index: round-1 behaviour); no pass graph
  // ---- where the result is stored (run_finalize)
  int stage_out = env_int("SNF_STAGE_OUT", -1);      // SNF_STAGE_OUT=0/1: result stored directly / staged through HBM; unset (< 0): staged while another pass is in flight
  bool stage_copy_kernel = env_is("SNF_STAGE_COPY", "kernel");   // SNF_STAGE_COPY=kernel: a staged result is copied by kernels inside the pass; default: two copies at the fetch
  // ---- timing and reports (b->timing / time_every / time_all start from these and change through snf_batch_set_timing / snf_batch_timing_every)
  bool prof = env_set("SNF_PROF");                   // SNF_PROF (set): [SNF_PROF] lines to stderr - stage counters, the forms a handle launches, the upload's split
  bool timing = !env_set("SNF_NO_TIMING");           // SNF_NO_TIMING (set): no HIP events around the kernels
  bool timeline = env_set("SNF_TIMELINE");           // SNF_TIMELINE (set): (offset, duration) of every bracketed op of the step to stderr; implies SNF_TIME_ALL; no pass graph
  bool time_all = env_set("SNF_TIME_ALL");           // SNF_TIME_ALL (set): HIP events around every launch, not only the heavy kernels; no pass graph
  int time_every = env_int("SNF_TIME_EVERY", 8);     // SNF_TIME_EVERY=n, default 8: event brackets on every n-th pass of the handle (negative: 0)
  std::string wg_trace_file = env_str("SNF_WG_TRACE_FILE");   // SNF_WG_TRACE_FILE=<path> (-DSNF_WG_TRACE builds, with SNF_PROF): every workgroup's class, start, duration
};

struct ProcessKnobs {
  int pace = env_int("SNF_PACE", 1);                 // SNF_PACE=0/1/2/3, default 1: the rules that keep passes in flight out of step - 0 off, 1 both, 2 copies in turn only, 3 spaced starts only
  double pace_frac = getenv("SNF_PACE_FRAC") ? atof(getenv("SNF_PACE_FRAC")) : 0.25;   // SNF_PACE_FRAC=f, default 0.25: spacing of pass starts as a fraction of the recent pass latency
  int gpu_slots = env_int("SNF_GPU_SLOTS", 0);       // SNF_GPU_SLOTS=n, default 0 (unbounded): at most n passes - of any process of this user - drive a device at a time
  size_t stage_arena_floor = getenv("SNF_STAGE_ARENA_MB") ? (size_t)atoll(getenv("SNF_STAGE_ARENA_MB")) << 20 : 0;   // SNF_STAGE_ARENA_MB=n: the pinned staging arena is never smaller (server.py)
  bool slab_cache = !env_set("SNF_NO_SLAB_CACHE");   // SNF_NO_SLAB_CACHE (set): no device-slab cache - every batch allocates and frees its own slabs
  bool stream_pool = !env_set("SNF_NO_STREAM_POOL"); // SNF_NO_STREAM_POOL (set): batches create and destroy their own HIP streams
  bool roctx = env_on("SNF_ROCTX");                  // SNF_ROCTX!=0: roctx ranges around the stages (libroctx64 is looked up at run time)
  int upload_threads = env_set("SNF_UPLOAD_THREADS") ? env_pos("SNF_UPLOAD_THREADS", 1) : 0;   // SNF_UPLOAD_THREADS=k (at least 1): host threads of the upload's staging pass; unset (0): the hardware's, 32 at most
};
// read at the first call; "once per process" is the intended meaning here
inline const ProcessKnobs& process_knobs() { static const ProcessKnobs k; return k; }

struct ExtractKnobs {   // read at every snf_extract_run
  bool thread_form = env_set("SNF_EXTRACT_THREAD");  // SNF_EXTRACT_THREAD (set): thread form of the extraction kernels (the reference's loops as they are)
  int waves = env_int("SNF_EXTRACT_WAVES", 4);       // SNF_EXTRACT_WAVES=4/5/6/8, default 4: waves/SIMD the wave form is compiled for (its register budget)
  int grid_cap = env_set("SNF_EXTRACT_GRID") ? env_pos("SNF_EXTRACT_GRID", 1) : (1 << 22);   // SNF_EXTRACT_GRID=n (at least 1), default 2^22:
                                                     //   a capped grid strides (measured, slower - the dispatcher balances unequal records better)
  bool xtrace_emit = env_is("SNF_XTRACE_PASS", "emit");   // SNF_XTRACE_PASS=emit (-DSNF_XTRACE builds): trace the emit pass; default: the counting pass
  std::string xtrace_out = env_str("SNF_XTRACE_OUT");     // SNF_XTRACE_OUT=<path> (-DSNF_XTRACE builds): the per-record trace is written there
};

struct BgzfKnobs {   // read at every snf_bgzf_inflate
  bool thread_form = env_set("SNF_BGZF_THREAD");     // SNF_BGZF_THREAD (set): a thread per BGZF member, its window in HBM (the second implementation the tests compare)
  int grid_cap = env_set("SNF_BGZF_GRID") ? env_pos("SNF_BGZF_GRID", 1) : (1 << 20);   // SNF_BGZF_GRID=n (at least 1), default 2^20: the inflate grid; beyond it a wave takes several members
};

struct BaiKnobs {   // read at every snf_bai_run
  bool thread_form = env_set("SNF_BAI_THREAD");      // SNF_BAI_THREAD (set): a thread per record in bai_span / bai_linear (the second implementation the tests compare)
  int grid_cap = env_set("SNF_BAI_GRID") ? env_pos("SNF_BAI_GRID", 1) : (1 << 20);   // SNF_BAI_GRID=n (at least 1), default 2^20: the grid of the wave forms; beyond it a wave takes several records
};

struct DeflateKnobs {   // read at every snf_deflate_run
  int grid_cap = env_set("SNF_DEFLATE_GRID") ? env_pos("SNF_DEFLATE_GRID", 1) : (1 << 20);   // SNF_DEFLATE_GRID=n (at least 1), default 2^20: the deflate grid; beyond it a workgroup takes several members
  int max_bits = [] { const int v = env_int("SNF_DEFLATE_MAXBITS", 15); return v >= 9 && v <= 15 ? v : 15; }();   // SNF_DEFLATE_MAXBITS=9..15, default 15 (deflate's limit; anything
                                                     //   else: 15): longest literal/length or distance code - tests lower it, so that ordinary inputs reach the limiter
};

struct FastaKnobs {   // read at every snf_fasta_index / snf_fasta_nruns / snf_fasta_fetch
  int grid_cap = env_set("SNF_FASTA_GRID") ? env_pos("SNF_FASTA_GRID", 1) : (1 << 20);   // SNF_FASTA_GRID=n (at least 1), default 2^20: the grids of fa_index / fa_nruns / fa_gather;
                                                     //   beyond it a workgroup takes several chunks, a wave several queries
};

struct CombineKnobs {   // read at every snf_combine_resolve_batch
  bool thread_form = env_set("SNF_COMBINE_THREAD");  // SNF_COMBINE_THREAD (set): thread form of the combine kernels
};

}  // namespace snf
