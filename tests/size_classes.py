"""The size thresholds at which the library changes kernel form, read from the sources by regular expression (the way
tests/test_knobs.py reads the switches), and the ladders t - 1, t, t + 1 the directed cases of tests/cases.py and
tests/test_size_classes.py are derived from.  A threshold that is no longer found is an error, not a default: a case that
silently tests the middle of a class is what this module is there to prevent.  ed_thresholds(): the same for the edit-distance
kernels and the merge kernel that calls them (tests/ed_edges.py, tests/test_edit_distance_edges.py).  extract_thresholds(): the same
for the extraction kernels (tests/extract_edges.py, tests/test_extract_edges.py).  coverage_thresholds(): the same for the read-table rank
index, the coverage kernels on it and the genotype table (tests/coverage_cases.py, tests/test_coverage_edges.py, tests/test_genotype_edges.py).
window_thresholds(): the same for the window front end and its packed fields (tests/window_cases.py, tests/test_window_edges.py).
merge_thresholds(): the same for the adaptive merge scan and the rule of its run cut (tests/merge_scan_cases.py, tests/test_merge_scan_edges.py)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sniffles_amd", "csrc")

# fixed by the machine / the kernels' shape, not by a named constant: a group of eight in d1g_refine<8> / d2g_call<8>, half a wave, a
# wave (d1w_refine / d2w_call: a lead per lane; e1w_finalize: SNF_E1_BATCH calls per wave), two waves, the 256-lead window instance,
# and the reference's own switch in compute_metrics (more than 100 leads)
GROUP, HALF_WAVE, WAVE, TWO_WAVES, WIN_MID, REF_METRICS = 8, 32, 64, 128, 256, 100


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text, re.M)
    if len(m) != 1:
        raise AssertionError(f"size_classes: expected exactly one match for {what} ({pattern!r}), found {len(m)}")
    return m[0]


def _define(name, header):
    return int(_one(r"^#define\s+" + name + r"\s+(\d+)\b", _src(header), name))


def thresholds():
    """dict of the named thresholds and of the literals of cons_class_of."""
    t = dict(
        big_stage_cap=_define("SNF_BIG_STAGE_CAP", "snf_wave_call.h"),
        big_final_cap=_define("SNF_BIG_FINAL_CAP", "snf_stage_final.h"),
        cons_small_l=_define("SNF_CONS_SMALL_L", "snf_stage_final.h"),
        cons_large_l=_define("SNF_CONS_LARGE_L", "snf_stage_final.h"),
        win_maxcap=_define("SNF_WIN_MAXCAP", "snf_stage_window.h"),
        heavy_n=int(_one(r'int\s+heavy_n\s*=\s*env_int\(\s*"SNF_HEAVY_N"\s*,\s*(\d+)\s*\)', _src("snf_knobs.h"), "the heavy_n default")),
        e1_batch=int(_one(r'int\s+e1_batch\s*=\s*env_int\(\s*"SNF_E1_BATCH"\s*,\s*(\d+)\s*\)', _src("snf_knobs.h"), "the e1_batch default")),
    )
    final = _src("snf_stage_final.h")
    m = re.search(r"SNF_HD int cons_class_of\(int wave_path, int klen, int skip, int64_t L, int32_t n_others\) \{\n(.*?)\n\}", final, re.S)
    if not m:
        raise AssertionError("size_classes: cons_class_of is no longer found in snf_stage_final.h")
    body = "\n".join(ln.split("//")[0] for ln in m.group(1).splitlines())
    g = _one(r"if \(!wave_path \|\| klen > (\d+) \|\| klen < 1 \|\| skip < 1 \|\| L >= (\d+)\) return 0;", body, "the guard of cons_class_of")
    s = _one(r"if \(npos <= (\d+) && n_others <= (\d+) && L <= SNF_CONS_SMALL_L && skip <= (\d+)\) return 1;", body, "the SMALL rule")
    l = _one(r"if \(npos <= (\d+) && n_others <= (\d+) && L <= SNF_CONS_LARGE_L\) return 2;", body, "the LARGE rule")
    r = _one(r"if \(npos <= (\d+) && n_others <= (\d+)\) return 4;", body, "the ROWS rule")
    t.update(cons_klen_max=int(g[0]), cons_l_end=int(g[1]), small_npos=int(s[0]), small_others=int(s[1]), small_skip=int(s[2]),
             large_npos=int(l[0]), large_others=int(l[1]), rows_npos=int(r[0]), rows_others=int(r[1]))
    return t


def ed_thresholds():
    """dict of the literals at which the edit-distance kernels (snf_myers.h / snf_myers.hip) and the merge kernel that calls them
    (snf_combine.hip) change form.  Both copies of a rule that is written twice are reported; that they agree is for the tests to say."""
    myers_h, myers, combine = _src("snf_myers.h"), _src("snf_myers.hip"), _src("snf_combine.hip")
    fits = _one(r"return \(64 \+ bd\.dl \+ 2 \* bd\.kk\) / 64 \+ 2 <= (\d+) \|\| \(m \+ 63\) / 64 <= (\d+);", myers_h,
                "the rule of ed_wave_band_fits")
    wide = _one(r"wide = !\(\(64 \+ bd\.dl \+ 2 \* bd\.kk\) / 64 \+ 2 <= (\d+) \|\| \(m \+ 63\) / 64 <= (\d+)\);", myers,
                "ed_batch's copy of the rule of ed_wave_band_fits")
    ed_grid = _one(r"hipLaunchKernelGGL\(ed_wave, dim3\(\(unsigned\)\(v\.n < (\d+) \? v\.n : (\d+)\)\)", myers, "the grid cap of ed_wave")
    cb_grid = _one(r"hipLaunchKernelGGL\(combine_problem_wave, dim3\(\(unsigned\)\(np < (\d+) \? np : (\d+)\)\)", combine,
                   "the grid cap of combine_problem_wave")
    for what, pair in (("the grid cap of ed_wave", ed_grid), ("the grid cap of combine_problem_wave", cb_grid)):
        if pair[0] != pair[1]:
            raise AssertionError(f"size_classes: {what} is written as two different numbers {pair}")
    return dict(
        thread_blocks=_define("SNF_ED_THREAD_BLOCKS", "snf_myers.hip"),
        small_blocks=int(_one(r"const bool small = \(m \+ 63\) / 64 <= (\d+);", myers, "the `small` rule of ed_batch")),
        band_blocks=int(fits[0]), band_pattern_blocks=int(fits[1]),
        host_band_blocks=int(wide[0]), host_band_pattern_blocks=int(wide[1]),
        ed_wave_grid=int(ed_grid[0]), combine_wave_grid=int(cb_grid[0]),
        carry_min_len=int(_one(r"k_off\[p \+ 1\] = k_off\[p\] \+ \(maxlen > (\d+) \? maxlen \+ 8 : 8\);", combine,
                               "the carry sizing rule of snf_combine_resolve_batch")),
    )


def extract_thresholds():
    """dict of the literals at which the extraction kernels (snf_extract.hip) change what a lane, a step, a chunk or a block holds, and
    of the defaults of the two switches that select the wave form's grid and instance (snf_knobs.h).  `step` is derived: the CIGAR
    operations a wave takes per step."""
    x, knobs = _src("snf_extract.hip"), _src("snf_knobs.h")
    clip = _one(r"const int k = lane < (\d+) \? lane : n_cig - 1 - \(lane - (\d+)\);\n\s*if \(lane < (\d+) \? k < n_cig : \(lane < (\d+) && k >= 1\)\)", x,
                "the clip lanes of extract_record")
    if not (clip[0] == clip[1] == clip[2]):
        raise AssertionError(f"size_classes: the lanes of the leading clip operations are written as different numbers {clip}")
    fold = _one(r"double a\[(\d+)\], nx\[(\d+)\];", x, "the registers of x_nmsum's fold")
    fold_step = _one(r"for \(int k0 = 0; k0 < cnt; k0 \+= (\d+)\) \{", x, "the step of x_nmsum's fold")
    if not (fold[0] == fold[1] == fold_step):
        raise AssertionError(f"size_classes: the width of x_nmsum's fold is written as different numbers {fold + (fold_step,)}")
    blocks = re.findall(r"hipLaunchKernelGGL\(x_(?:count|emit), dim3\(\(unsigned\)\(\(n \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\), 0, 0, v, n\);", x)
    if len(blocks) != 2:
        raise AssertionError(f"size_classes: expected the two thread-form launches of snf_extract.hip, found {len(blocks)}")
    sizes = {int(b[0]) + 1 for b in blocks} | {int(v) for b in blocks for v in b[1:]}
    if len(sizes) != 1:
        raise AssertionError(f"size_classes: the block size of the thread-form launches is written as different numbers {blocks}")
    opl = int(_one(r"constexpr int OPL = WAVE \? (\d+) : 1;", x, "OPL"))
    comma = _one(r"for \(int32_t k0 = ea; k0 < eb; k0 \+= (\d+)\) \{\n[^\n]*\n[^\n]*\n\s*if \(eb - k0 < (\d+)\) z &= \(1ull << \((\d+) \* \(eb - k0\)\)\) - 1ull;", x,
                 "the word of the comma scanner")
    if len(set(comma)) != 1:
        raise AssertionError(f"size_classes: the word of the comma scanner is written as different numbers {comma}")
    launch = re.search(r"template <bool EMIT> void x_launch_wave\(int waves, unsigned grid, const ExView& v, int64_t n\) \{\n(.*?)\n\}", x, re.S)
    if not launch:
        raise AssertionError("size_classes: x_launch_wave is no longer found in snf_extract.hip")
    instances = [int(w) for w in re.findall(r"x_wave<EMIT, (\d+)>", launch.group(1))]
    if len(instances) < 2 or len(set(instances)) != len(instances):
        raise AssertionError(f"size_classes: the instances of x_launch_wave read as {instances}")
    return dict(
        comma_word=int(comma[0]), wave_instances=tuple(sorted(instances)),
        nul_chunk=int(_one(r"x_find_nul\(const uint8_t\* blob, int64_t p, int64_t end, int lane\) \{\n\s*const int W = WAVE \? (\d+) : 1;\n\s*for \(int64_t q = p; q < end; q \+= W\)",
                           x, "the chunk of x_find_nul")),
        xmaxseg=_define("XMAXSEG", "snf_extract.hip"), xauxcap=_define("XAUXCAP", "snf_extract.hip"),
        nm_chunk=_define("X_NM_CHUNK", "snf_extract.hip"), ahead=_define("X_AHEAD", "snf_extract.hip"),
        opl=opl, step=WAVE * opl,
        sa_chunk=int(_one(r"for \(int32_t c0 = 0; c0 <= sa_len; c0 \+= (\d+)\) \{", x, "the chunk of the SA cutter")),
        clip_lanes=int(clip[0]), clip_lanes_end=int(clip[3]),
        nm_fold=int(fold_step), thread_block=sizes.pop(),
        blob_pad=int(_one(r"v\.blob = x_up\(x->dev, in->records, \(size_t\)in->records_len, (\d+)\);", x, "the blob padding of do_upload")),
        grid_cap=1 << int(_one(r'int grid_cap = env_set\("SNF_EXTRACT_GRID"\) \? env_pos\("SNF_EXTRACT_GRID", 1\) : \(1 << (\d+)\);', knobs,
                               "the default grid cap of the wave form")),
        waves=int(_one(r'int waves = env_int\("SNF_EXTRACT_WAVES", (\d+)\);', knobs, "the default of SNF_EXTRACT_WAVES")),
    )


def coverage_thresholds():
    """dict of the sizes of the read-table rank index (snf_exact.h: every 2^SNF_TOP_SHIFT-th global position is sampled), of the chunks of
    the coverage sums (snf_wave_call.h: reads per workgroup round of d5w_covsum, the kernel every pass launches - the literal of the
    kernel and the two of its grid in snf_lib.hip have to agree; snf_stage_call.h: positions per thread of d5x_covexact, and
    SNF_COV_CHUNK of d5_covsum, a thread form that is instantiated and launched by nothing), of the depth from which a task takes the
    exact walk (the uint16 wrap decision of the upload, snf_lib.hip) and of the side of the genotype table (snf_view.h)."""
    lib_hip = _src("snf_lib.hip")
    ch = _one(r"__global__ void __launch_bounds__\(256\) d5w_covsum\(const View v, int64_t n_unused\) \{\n[^\n]*\n[^\n]*\n\s*const int64_t CH = (\d+);",
              _src("snf_wave_call.h"), "the chunk of d5w_covsum")
    grid = _one(r"int64_t grid = \(R \+ (\d+)\) / (\d+); if \(grid > \d+\) grid = \d+;\n\s*hipLaunchKernelGGL\(d5w_covsum,", lib_hip, "the grid of d5w_covsum")
    if not (int(ch) == int(grid[0]) + 1 == int(grid[1])):
        raise AssertionError(f"size_classes: the chunk of d5w_covsum is written as different numbers {(ch,) + tuple(grid)}")
    if len(re.findall(r"\bd5_covsum\b", lib_hip)) != 1:
        raise AssertionError("size_classes: d5_covsum is no longer named exactly once (its instantiation) in snf_lib.hip - if it is launched, it needs cases")
    return dict(
        covsum_chunk=int(ch),
        top_shift=_define("SNF_TOP_SHIFT", "snf_exact.h"),
        cov_chunk=_define("SNF_COV_CHUNK", "snf_stage_call.h"),
        covx_chunk=_define("SNF_COVX_CHUNK", "snf_stage_call.h"),
        gt_n=_define("SNF_GT_N", "snf_view.h"),
        wrap_depth=int(_one(r"if \(masked \|\| maxd\[\(size_t\)t\] >= (\d+) \|\| b->k\.cov_exact\)", lib_hip, "the uint16 wrap decision of the upload")),
    )


def window_thresholds():
    """dict of the literals of the window front end (snf_stage_window.h, the width choice of do_upload in snf_lib.hip, the two width
    switches of snf_knobs.h): the largest instance, the widths tried, the 256 and 64 of the width / instance rule, the pad behind the
    sort keys, and every shift and mask of the packed fields - the bin of a lead inside its window and `is_long` / `hap` next to it
    (win_pack), the sort key (wkey_make), the high half of a key_out word, whead2 - with the relations between them the kernels rely
    on.  A field that is written with one literal and read with another is an error here, like a literal that is no longer found."""
    w, lib_hip, knobs = _src("snf_stage_window.h"), _src("snf_lib.hip"), _src("snf_knobs.h")
    pack = _one(r"SNF_HD uint32_t win_pack\(const View& v, uint32_t bin_low, bool is_long, uint32_t hap\) \{ return bin_low \| "
                r"\(\(is_long \? 1u : 0u\) << (\d+)\) \| \(hap << (\d+)\); \}", w, "win_pack")
    unpack = (_one(r"SNF_HD uint32_t win_bin_low\(uint32_t a\) \{ return a & (0x[0-9a-f]+)u; \}", w, "win_bin_low"),
              _one(r"SNF_HD bool win_is_long\(uint32_t a\) \{ return \(a >> (\d+)\) & 1u; \}", w, "win_is_long"),
              _one(r"SNF_HD uint32_t win_hap\(uint32_t a\) \{ return \(a >> (\d+)\) & 3u; \}", w, "win_hap"))
    key = _one(r"return \(\(uint64_t\)widx << (\d+)\) \| \(\(uint64_t\)win_bin_low\(a\) << (\d+)\) \| \(\(uint64_t\)\(uint32_t\)word << (\d+)\) \| "
               r"\(\(uint64_t\)win_hap\(a\) << (\d+)\) \| \(win_is_long\(a\) \? 1ull : 0ull\);", w, "wkey_make")
    unkey = (_one(r"wkey_group\(uint64_t k\) \{ return \(uint32_t\)\(k >> (\d+)\); \}", w, "wkey_group"),
             _one(r"wkey_bin\(uint64_t k\) \{ return \(uint32_t\)\(k >> (\d+)\) & (0x[0-9a-f]+)u; \}", w, "wkey_bin"),
             _one(r"wkey_widx\(uint64_t k\) \{ return \(uint32_t\)\(k >> (\d+)\); \}", w, "wkey_widx"),
             _one(r"wkey_index\(uint64_t k\) \{ return \(uint32_t\)\(k >> (\d+)\); \}", w, "wkey_index"),
             _one(r"wkey_hap\(uint64_t k\) \{ return \(uint32_t\)\(k >> (\d+)\) & 3u; \}", w, "wkey_hap"))
    hi = _one(r"\(\(f_norm \? rn : rl\) << (\d+)\) \| \(\(uint32_t\)j << (\d+)\) \| \(f_seed \? rs << (\d+) : 0u\);", w, "the high half of key_out")
    unhi = (_one(r"const int64_t owner = p / 64 - \(int64_t\)\(\(hi >> (\d+)\) & (\d+)u\);", w, "the owner of a position in w6t_emit"),
            _one(r"const uint32_t rank = \(hi >> (\d+)\) & (0x[0-9a-f]+)u;", w, "the rank of a lead in w6t_emit"),
            _one(r"const int64_t qs = \(int64_t\)v\.ws_seeds\[owner\] \+ \(hi >> (\d+)\);", w, "the seed rank in w6t_emit"))
    h2 = _one(r"v\.whead2\[B0 \+ x\] = \(uint64_t\)\(uint32_t\)\(int32_t\)start \| \(\(uint64_t\)wG\[wl\] << (\d+)\) \| \(\(uint64_t\)\(f_norm \? rl : rn\) << (\d+)\);", w, "whead2")
    unh2 = (_one(r"const uint32_t other = \(uint32_t\)\(h2 >> (\d+)\);", w, "the other offset in w6t_emit"),
            _one(r"v\.seed_grp\[qs\] = \(int\)\(\(h2 >> (\d+)\) & (0x[0-9a-f]+)u\);", w, "seed_grp in w6t_emit"))
    rows = _one(r"constexpr int CAPW = CAP \+ (\d+), E = CAPW / (\d+), PAD = (\d+);", w, "the rows of w4s_segment")
    wmin = _one(r"const int WIN_W_MAX = b->k\.win_bits_max, WIN_W_MIN = (\d+);", lib_hip, "WIN_W_MIN")
    wmax = _one(r'int win_bits_max = \[\] \{ const int v = env_int\("SNF_WIN_BITS_MAX", (\d+)\); return v >= (\d+) && v <= (\d+) \? v : (\d+); \}\(\);',
                knobs, "the default and the range of SNF_WIN_BITS_MAX")
    pick = _one(r"if \(hc\.max_win <= (\d+) \|\| \(best_w < 0 && hc\.max_win <= SNF_WIN_MAXCAP\)\) \{[^\n]*\n\s*if \(hc\.max_win <= (\d+)\) break;", lib_hip,
                "the width rule of do_upload")
    cap = _one(r"b->win_cap = best_max <= (\d+) \? (\d+) : best_max <= (\d+) \? (\d+) : SNF_WIN_MAXCAP;", lib_hip, "the instance rule of do_upload")
    front = _one(r"const bool front_wanted = v\.prefilter && v\.wave_path && b->k\.winfront && b->k\.fuse && N <= \(\(int64_t\)1 << (\d+)\) && T < \(1 << (\d+)\);",
                 lib_hip, "front_wanted")
    t = dict(
        win_maxcap=_define("SNF_WIN_MAXCAP", "snf_stage_window.h"), w_min=int(wmin), w_max_default=int(wmax[0]), w_max_lo=int(wmax[1]), w_max_hi=int(wmax[2]),
        win_mid=int(pick[0]), win_small=int(cap[0]), pad=int(rows[2]),
        long_shift=int(pack[0]), hap_shift=int(pack[1]), bin_mask=int(unpack[0], 16),
        key_widx_shift=int(key[0]), key_bin_shift=int(key[1]), key_index_shift=int(key[2]), key_hap_shift=int(key[3]),
        hi_rank_shift=int(hi[0]), hi_blk_shift=int(hi[1]), hi_seed_shift=int(hi[2]), hi_rank_mask=int(unhi[1][1], 16), hi_blk_mask=int(unhi[0][1]),
        h2_grp_shift=int(h2[0]), h2_other_shift=int(h2[1]), h2_grp_mask=int(unh2[1][1], 16),
        n_bits=int(front[0]), t_bits=int(front[1]),
    )
    same = [("the default of SNF_WIN_BITS_MAX and its fall-back", wmax[0], wmax[3]), ("the 256 of the width rule", pick[0], pick[1]),
            ("the 256 of the instance rule", pick[0], cap[2]), ("the 256 of the instance rule", cap[2], cap[3]), ("the 64 of the instance rule", cap[0], cap[1]),
            ("the rows of w4s_segment", rows[0], rows[1]), ("is_long", pack[0], unpack[1]), ("hap", pack[1], unpack[2]),
            ("the bin of a key", key[1], unkey[0]), ("the bin of a key", key[1], unkey[1][0]), ("the bin mask", unpack[0], unkey[1][1]),
            ("the window of a key", key[0], unkey[2]), ("the index of a key", key[2], unkey[3]), ("the hap of a key", key[3], unkey[4]),
            ("the rank of a word", hi[0], unhi[1][0]), ("the block distance of a word", hi[1], unhi[0][0]), ("the seed rank of a word", hi[2], unhi[2]),
            ("the group of whead2", h2[0], unh2[1][0]), ("the other offset of whead2", h2[1], unh2[0])]
    for what, a, b in same:
        if int(a, 0) != int(b, 0):
            raise AssertionError(f"size_classes: {what} is written as two different numbers ({a}, {b})")
    # ---- what the kernels rely on
    top = WAVE - 1 + t["win_maxcap"]                       # the last position a wave of w4s_segment can own, relative to its block
    rel = [
        ("the bin mask is a run of low bits below is_long", t["bin_mask"] & (t["bin_mask"] + 1) == 0 and t["bin_mask"] + 1 == 1 << t["long_shift"]),
        ("hap lies above is_long", t["hap_shift"] == t["long_shift"] + 1),
        ("the widest admissible W fits the bin field", (1 << t["w_max_hi"]) - 1 <= t["bin_mask"]),
        ("the widths tried begin at WIN_W_MIN", t["w_max_lo"] == t["w_min"] <= t["w_max_default"] <= t["w_max_hi"]),
        ("the bin field of a key ends below the window", t["key_bin_shift"] + t["bin_mask"].bit_length() <= t["key_widx_shift"]),
        ("the window index of a wave (64 windows) fits above it", t["key_widx_shift"] + 6 <= 64),
        ("hap (2 bits) and is_long lie below the index", t["key_hap_shift"] == 1 and t["key_index_shift"] == t["key_hap_shift"] + 2),
        ("25 + 3 index bits lie below the bin of a key", t["n_bits"] + t["key_index_shift"] <= t["key_bin_shift"]),
        ("63 + SNF_WIN_MAXCAP fits the rank field", top <= t["hi_rank_mask"] and t["hi_rank_shift"] + t["hi_rank_mask"].bit_length() <= t["hi_blk_shift"]),
        ("... and uint16_t (hpos, the counts of whead)", top < 1 << 16),
        ("(63 + SNF_WIN_MAXCAP) / 64 fits the block-distance field", top // WAVE <= t["hi_blk_mask"] and
         t["hi_blk_shift"] + t["hi_blk_mask"].bit_length() <= t["hi_seed_shift"] and t["hi_blk_mask"] & (t["hi_blk_mask"] + 1) == 0),
        ("the seed-rank field holds 63 + SNF_WIN_MAXCAP", top < 1 << (32 - t["hi_seed_shift"])),
        ("the flags lie below the rank", t["hi_rank_shift"] == 4),
        ("the other offset of whead2 holds 63 + SNF_WIN_MAXCAP", top < 1 << (64 - t["h2_other_shift"])),
        ("the group of whead2 lies between the start and the other offset", t["h2_grp_shift"] == 32 and
         t["h2_grp_shift"] + t["h2_grp_mask"].bit_length() <= t["h2_other_shift"]),
        ("t * 8 + svtype fits the group of whead2", (((1 << t["t_bits"]) - 1) * 8 + 7) <= t["h2_grp_mask"]),
        ("the instances ascend", WAVE == t["win_small"] < t["win_mid"] == WIN_MID < t["win_maxcap"]),
        ("the pad is a power of two that divides a block", t["pad"] & (t["pad"] - 1) == 0 and WAVE % t["pad"] == 0),
    ]
    for what, ok in rel:
        if not ok:
            raise AssertionError(f"size_classes: {what} - no longer true of the literals as read: {t}")
    return t


def merge_thresholds():
    """dict of the literals of the adaptive merge scan (snf_stage_cluster.h: compute_metrics, merge_walk, c4_emit) and of the rule
    that resolves its run cut (snf_lib.hip: do_upload).  The reference's sample cap is written twice (where the leads are read and
    where the sums are added), the bound of the added sums three times; a copy with another value is an error, like a literal that
    is no longer found."""
    c, lib_hip = _src("snf_stage_cluster.h"), _src("snf_lib.hip")
    cap = _one(r"int64_t n = len < (\d+) \? len : (\d+);", c, "the sample cap of compute_metrics")
    cap_added = _one(r"const int64_t nn_ = Lm < (\d+) \? Lm : (\d+);", c, "the sample cap of the added sums (merge_walk)")
    added = _one(r"if \(!v\.merge_reread && Lm < (\d+) && A\.cs\.s2 != ~0ull && B\.cs\.s2 != ~0ull && A\.cs\.hi == B\.lo\) \{", c, "the rule of the added sums")
    mch = _one(r"constexpr int MCH = (\d+);", c, "MCH")
    wide = _one(r"wide \|= \(uint64_t\)\(d < 0 \? -d : d\) >> (\d+);", c, "the switch to 128-bit sums")
    fits = _one(r"const bool fits = S2m < \(\(i128\)1 << (\d+)\) && S1m < \(\(i128\)1 << (\d+)\) && S1m > -\(\(i128\)1 << (\d+)\);", c, "the bound of the added sums")
    hand = _one(r"if \(hd\.n > (\d+)\) \{ hand_c = ", c, "the hand-over size of c4_emit")
    cut = _one(r"cut = inner > v\.run_gap;", c, "the run cut of b1_seedmetrics_body")
    base = _one(r"const int gap_base = b->cfg\.cluster_merge_bnd > gap_int\(b->cfg\.cluster_repeat_h_max\) \? b->cfg\.cluster_merge_bnd : gap_int\(b->cfg\.cluster_repeat_h_max\);",
                lib_hip, "the base of run_gap (the larger of cluster_merge_bnd and cluster_repeat_h_max)")
    gap = _one(r"v\.run_gap = b->k\.run_gap != KNOB_UNSET \? b->k\.run_gap : \(gap_base > (\d+) \? gap_base : (\d+)\);", lib_hip, "the floor of run_gap")
    clamp = _one(r"static int gap_int\(double x\) \{ return !\(x > 0\.0\) \? 0 : x >= (\d+)\.0 \? (\d+) : \(int\)x; \}", lib_hip, "the clamp of run_gap's cast")
    assert cut and base
    same = [("the sample cap of compute_metrics", cap[0], cap[1]), ("the sample cap of the added sums", cap_added[0], cap_added[1]),
            ("the sample cap where the leads are read and where the sums are added", cap[0], cap_added[0]),
            ("the bound of the added sums", fits[0], fits[1]), ("the bound of the added sums", fits[1], fits[2]),
            ("the floor of run_gap", gap[0], gap[1]), ("the clamp of run_gap's cast", clamp[0], clamp[1])]
    for what, a, b in same:
        if int(a) != int(b):
            raise AssertionError(f"size_classes: {what} is written as two different numbers ({a}, {b})")
    t = dict(sample_cap=int(cap[0]), added_below=int(added), mch=int(mch), wide_shift=int(wide), fits_shift=int(fits[0]), run_gap_floor=int(gap[0]),
             run_gap_max=int(clamp[0]), hand_over=int(hand))
    rel = [
        ("the sample cap is the reference's (compute_metrics, max_n = 100)", t["sample_cap"] == REF_METRICS),
        ("the sums are added below the first length whose step is 2", t["added_below"] == 2 * t["sample_cap"] and t["added_below"] // t["sample_cap"] == 2
         and (t["added_below"] - 1) // t["sample_cap"] == 1),
        ("the squares of added_below - 1 deviations below 2^wide_shift stay below the bound of the added sums",
         (t["added_below"] - 1) * ((1 << t["wide_shift"]) - 1) ** 2 < 1 << t["fits_shift"]),
        ("... and twice the bound fits int64_t / uint64_t (two parts, each below it, are added before the check)", t["fits_shift"] + 1 <= 63),
        ("a batch of requests is shorter than the sample cap", 1 < t["mch"] < t["sample_cap"]),
        ("the clamp of run_gap's cast fits int32_t", t["run_gap_max"] < 1 << 31),
        ("clusters up to a group of eight stay with d1g_refine<8>", t["hand_over"] == GROUP),
    ]
    for what, ok in rel:
        if not ok:
            raise AssertionError(f"size_classes: {what} - no longer true of the literals as read: {t}")
    return t


def ed_band_is_wide(t, m, n, k):
    """not ed_wave_band_fits(m, n, k), from the literals as read (m <= n; k < 0: no cut-off): the pair takes the multi-pass form."""
    dl = n - m
    if k >= 0 and dl > k:
        return False
    kk = m if k < 0 else (k - dl) // 2
    return not ((64 + dl + 2 * kk) // 64 + 2 <= t["band_blocks"] or (m + 63) // 64 <= t["band_pattern_blocks"])


def cons_npos(L, klen, skip):
    """snf_stage_final.h::cons_npos - sampled positions of a best read of L bases."""
    m = L - klen
    return 0 if m <= 0 else (m + skip - 1) // skip


def cons_class(t, klen, skip, L, n_others):
    """cons_class_of on the wave path, from the literals as read: 1 SMALL, 2 LARGE, 4 ROWS, 0 the thread kernels."""
    if klen > t["cons_klen_max"] or klen < 1 or skip < 1 or L >= t["cons_l_end"]:
        return 0
    npos = cons_npos(L, klen, skip)
    if npos <= t["small_npos"] and n_others <= t["small_others"] and L <= t["cons_small_l"] and skip <= t["small_skip"]:
        return 1
    if npos <= t["large_npos"] and n_others <= t["large_others"] and L <= t["cons_large_l"]:
        return 2
    if npos <= t["rows_npos"] and n_others <= t["rows_others"]:
        return 4
    return 0


def around(*ts):
    """t - 1, t, t + 1 for every threshold, ascending, without repeats."""
    return sorted({x for t in ts for x in (t - 1, t, t + 1)})


def ladder_sizes(with_window_cap=False):
    """Lead counts of a cluster-size ladder: both sides of every size class of the cluster kernels (and 2 / 3, the smallest clusters
    there are).  with_window_cap: also the largest window the front end takes (one ladder only: 3 000 leads more)."""
    t = thresholds()
    s = {2, 3} | set(around(GROUP, t["heavy_n"], HALF_WAVE, WAVE, TWO_WAVES, t["big_stage_cap"], WIN_MID, t["big_final_cap"]))
    s |= {WAVE + 2, REF_METRICS, REF_METRICS + 1}
    if with_window_cap:
        s |= set(around(t["win_maxcap"]))
    return sorted(s)
