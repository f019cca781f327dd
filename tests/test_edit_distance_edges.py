"""The bit-parallel Myers kernels (snf_myers.h, snf_myers.hip) at their form edges, through both callers: the tested entry point
(snf_edit_distance_batch_k, which sends every pattern of at most SNF_ED_THREAD_BLOCKS blocks to the thread form) and the merge kernel
(combine_problem_wave, which calls the wave forms for EVERY length: short patterns, texts shorter than one 8-column group, equal strings
of a few bytes, and the multi-pass fallback on its per-problem carry rows are reached only there).

Inside the merge only "d <= kmax or not" shows, and only as group membership, so tests/ed_edges.py builds merge problems that read the
predicate d(A, B) <= k for any chosen k (the probe).  Every probe test asserts three things: membership against the exact two-row DP
of the C oracle, the whole out_group against oracle.combine_resolve on the same packed problem, and that the kernel's alignment counter
equals the number of probes (a probe a gate had rejected would never have aligned).  Distances are integers: every comparison is exact.
All lengths and cut-offs come from the literals tests/size_classes.py reads out of the sources.

Tiers: every case runs under `-m gpu`; the probe and batch cases have a host-tier twin (tests/emu) over a reduced set; the second
round of the grid-stride loops and the thread form of the merge (SNF_COMBINE_THREAD) are GPU-only."""
import ctypes as C

import numpy as np
import pytest

import ed_edges as ee
import size_classes as sc
from sniffles_amd import abi, lib
from sniffles_amd.config import SnifflesConfig

E = ee.E
TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]
PROBE_CFG = SnifflesConfig(combine_pctseq=ee.PROBE_PCTSEQ)
_dp_cache = {}


def use_tier(tier):
    if tier == "host":
        import emu.emu as EM
        EM.lib()                                         # the host tier becomes the library of this test
    else:
        assert lib.device_count() >= 1


def dp(oracle_mod, a, b):
    """The reference of every case: the exact DP, once per pair and session."""
    if (a, b) not in _dp_cache:
        _dp_cache[(a, b)] = oracle_mod.edit_distance(a, b)
    return _dp_cache[(a, b)]


def run_probes(cases, oracle_mod, cfg=PROBE_CFG, replay=True):
    """cases: [(A, B, k, form)], one batch.  Returns the out_group of every probe.  replay=False: without the oracle's replay of the
    packed problems (for a second run of cases whose first run had it)."""
    keep = []
    packed = [ee.probe(a, b, k, form, keep) for a, b, k, form in cases]
    lib.combine_resolve_batch(cfg, [p[0] for p in packed])
    stats = lib.combine_last_stats()
    got = [p[1].tolist() for p in packed]
    ds = [dp(oracle_mod, a, b) for a, b, _, _ in cases]
    wrong = [(i, form, len(a), len(b), k, d, g) for i, ((a, b, k, form), (_, _, yes, no), d, g) in enumerate(zip(cases, packed, ds, got))
             if g != (yes if d <= k else no)]
    assert wrong == [], f"(index, form, len A, len B, k, d, out_group) of {len(wrong)} / {len(cases)} probes: {wrong[:8]}"
    for (q, out, _, _), g in zip(packed if replay else [], got):
        oracle_mod.combine_resolve(cfg, q)               # (writes the same out_group array)
        assert out.tolist() == g
    assert stats["alignments"] == len(cases)
    return got


# ---------------------------------------------------------------------------------------------- E. the thresholds themselves
def test_ed_thresholds_are_found_and_their_copies_agree():
    for k, v in E.items():
        assert isinstance(v, int) and v > 0, k
    assert E["thread_blocks"] == E["small_blocks"]                                   # the LDS rows of ed_thread_lds hold what ed_batch sends it
    assert (E["band_blocks"], E["band_pattern_blocks"]) == (E["host_band_blocks"], E["host_band_pattern_blocks"])   # carry bytes where the kernel wants them
    assert E["band_blocks"] < sc.WAVE and E["band_pattern_blocks"] < sc.WAVE         # a lane per block of the band, and one to spare
    assert E["carry_min_len"] <= ee.ROT                                              # every pattern of more than 63 blocks has its carry row
    for m, n, k, wide in ((ee.ROT + 1, ee.ROT + 1, ee.BAND_EDGE - 1, False), (ee.ROT + 1, ee.ROT + 1, ee.BAND_EDGE, True),
                          (ee.ROT, ee.ROT, -1, False), (ee.ROT + 1, ee.ROT + 1, -1, True), (ee.ROT + 1, ee.ROT + 2, ee.BAND_EDGE, False),
                          (ee.ROT + 1, ee.ROT + 2, ee.BAND_EDGE + 1, True), (ee.ROT + 1, 3 * ee.ROT, 10, False)):
        assert sc.ed_band_is_wide(E, m, n, k) == wide, (m, n, k)


@pytest.mark.parametrize("literal", ["SNF_ED_THREAD_BLOCKS", "const bool small", f"<= {E['band_pattern_blocks']};", "wide = !(",
                                     f"v.n < {E['ed_wave_grid']}", f"np < {E['combine_wave_grid']}", f"maxlen > {E['carry_min_len']}"])
def test_a_missing_ed_threshold_is_an_error(literal, monkeypatch):
    real = sc._src
    assert any(literal in real(f) for f in ("snf_myers.h", "snf_myers.hip", "snf_combine.hip"))
    monkeypatch.setattr(sc, "_src", lambda name: real(name).replace(literal, "/* gone */"))
    with pytest.raises(AssertionError):
        sc.ed_thresholds()


# ---------------------------------------------------------------------------------------------- A. the probe, through the merge kernel
@pytest.mark.parametrize("tier", TIERS)
def test_probe_short_pairs(tier, oracle_mod):
    """Patterns of 0 .. 9 blocks against texts 0, 1, 7, 8, 9 bytes longer, every wave form of ed_wave_pair_k_any: what
    snf_edit_distance_batch never sends to a wave."""
    use_tier(tier)
    pairs = ee.short_pairs()
    assert {k for k, _, _ in pairs} == {"symbolic", "acgt", "text_other", "planes"}
    assert {min(len(a), len(b)) for _, a, b in pairs} >= set(ee.SHORT_M) and {abs(len(a) - len(b)) for _, a, b in pairs} == set(ee.SHORT_DL)
    cases = [(a, b, k, form) for _, a, b in pairs for k in ee.short_ks(a, b, dp(oracle_mod, a, b)) for form in ee.FORMS]
    run_probes(cases, oracle_mod)
    joined = sum(dp(oracle_mod, a, b) <= k for a, b, k, _ in cases)
    assert len(cases) // 4 < joined < 3 * len(cases) // 4


@pytest.mark.parametrize("tier", TIERS)
def test_probe_identical_strings_shortcut(tier, oracle_mod):
    """Equal lengths: the untouched pair is accepted at k = 0 (the shortcut, or the alignment behind it); one substitution in the first
    or last byte of an 8-byte word, of a 512-byte round or of the tail is rejected at k = 0 and accepted at k = 1."""
    use_tier(tier)
    pairs = ee.shortcut_pairs()
    assert {len(a) for a, _, _ in pairs} == set(ee.SHORTCUT_M)
    cases = []
    for a, b, d in pairs:
        assert dp(oracle_mod, a, b) == d and len(a) == len(b) and (a is not b)
        cases += [(a, b, k, form) for k in ((0,) if d == 0 else (0, 1)) for form in ee.FORMS]
    run_probes(cases, oracle_mod)


def interleaved(long_cases, form):
    """The long probes with a short problem behind each (maxlen 5 / 4000 / 4001 in turn): a carry row that is mis-offset or overlaps
    its neighbour's changes a result."""
    out = []
    for i, (a, b, k) in enumerate(long_cases):
        out.append((a, b, k, form))
        out.append(ee.filler(i) + (form,))
    return out


@pytest.mark.parametrize("form", ee.FORMS)
@pytest.mark.parametrize("m", [ee.ROT] + ee.WIDE_M)
@pytest.mark.gpu
def test_probe_band_fit_edge_and_multi_pass_gpu(m, form, oracle_mod):
    """k = 3902 .. 3905 x d = k - 1, k, k + 1 (d by construction) x n - m = 0, 1: dl + 2 kk = 3903 | 3904 with 63 blocks (always the
    banded wave form) and with more (the multi-pass ed_wave_pair on the problem's own carry row from 3904 on)."""
    use_tier("gpu")
    cases = ee.wide_cases(m)
    for a, b, k in cases[::4] + cases[1::4] + cases[2::4]:
        d = dp(oracle_mod, a, b)
        assert d == len(b) - len(a) + sum(x in b"GT" for x in b[:len(a)]) and k - 1 <= d <= k + 1          # the construction holds
    assert any(sc.ed_band_is_wide(E, len(a), len(b), k) for a, b, k in cases) == (m > ee.ROT)
    run_probes(interleaved(cases, form), oracle_mod)


@pytest.mark.parametrize("alphabet", sorted(ee.ALPHABETS))
def test_probe_multi_pass_host(alphabet, oracle_mod):
    """Host twin of the above, one batch per alphabet: both sides of the band rule at k = 3903 | 3904 (n = m) and 3904 | 3905 (n = m + 1),
    d = k and k + 1, two long problems around a short one with maxlen 4000 and one with 4001."""
    use_tier("host")
    form = ee.FORMS[sorted(ee.ALPHABETS).index(alphabet) % 2]
    cases = [c for c in ee.wide_cases(ee.WIDE_M[0], alphabet)
             if c[2] - (len(c[1]) - len(c[0])) in (ee.BAND_EDGE - 1, ee.BAND_EDGE) and dp(oracle_mod, c[0], c[1]) in (c[2], c[2] + 1)]
    assert len(cases) == 8 and sum(sc.ed_band_is_wide(E, len(a), len(b), k) for a, b, k in cases) == 4
    batch = interleaved(cases[:4], form) + interleaved(cases[4:], form)      # (the fillers of both halves: 5 bytes, 4000, 5, 5 - so:)
    batch[-1] = ee.filler(5) + (form,)
    assert {max(len(a), len(b)) for a, b, _, _ in batch} >= {E["carry_min_len"], E["carry_min_len"] + 1}
    run_probes(batch, oracle_mod)


@pytest.mark.gpu
def test_probe_multi_pass_bit_plane_alphabet_gpu(oracle_mod):
    use_tier("gpu")
    run_probes(interleaved(ee.wide_cases(ee.WIDE_M[0], "planes"), "pair"), oracle_mod)


@pytest.mark.gpu
def test_default_pctseq_needs_the_multi_pass_form_at_14kb_gpu(oracle_mod):
    """The default combine_pctseq (0.7) on 14-kb ALTs: the kernel's own cut-off (4199) is wider than the wave, so the product
    configuration reaches the multi-pass form; d = 4199 joins, d = 4200 does not, a short problem between the two."""
    use_tier("gpu")
    cfg, ln = SnifflesConfig(), 14000
    kmax = max(d for d in range(ln) if (ln - d) / ln > cfg.combine_pctseq)
    assert sc.ed_band_is_wide(E, ln, ln, kmax)
    keep, packed, exp = [], [], []
    for i, d in enumerate((kmax, kmax + 1)):
        a, b = ee.constructed(ln, 0, d)
        assert dp(oracle_mod, a, b) == d
        for form in ee.FORMS:
            q, out, yes, no = ee.probe(a, b, None, form, keep, ln=ln)
            packed.append((q, out))
            exp.append(yes if d <= kmax else no)
            q, out, yes, no = ee.probe(*ee.filler(i)[:2], None, form, keep, ln=ee.filler(i)[2] * 40)
            packed.append((q, out))
            exp.append(yes)
    lib.combine_resolve_batch(cfg, [q for q, _ in packed])
    stats = lib.combine_last_stats()
    got = [out.tolist() for _, out in packed]
    assert got == exp
    for (q, out), g in zip(packed, got):
        oracle_mod.combine_resolve(cfg, q)
        assert out.tolist() == g
    assert stats["alignments"] == len(packed)


def rotating_cases(oracle_mod):
    out = []
    for m in ee.ROTATING_M:
        for planes in (False, True):
            a, b = ee.near(m, m % 2, planes)
            d = dp(oracle_mod, a, b)
            assert 20 <= d <= 60
            out += [(a, b, k) for k in (d - 1, d, d + 1)]
    return out


@pytest.mark.parametrize("tier", TIERS)
def test_probe_rotating_band(tier, oracle_mod):
    """63 .. 66 pattern blocks and a narrow band (d ~ 40, k = d - 1, d, d + 1): where lane 0 starts to hold block 64 after block 0, in
    the eight-column form and in the bit-plane form."""
    use_tier(tier)
    cases = rotating_cases(oracle_mod)
    assert not any(sc.ed_band_is_wide(E, min(len(a), len(b)), max(len(a), len(b)), k) for a, b, k in cases)
    batch = [c + (ee.FORMS[i % 2],) for i, c in enumerate(cases)]
    if tier == "gpu":                                                        # (the host tier: every pair and cut-off, the forms in turn)
        batch += [c + (ee.FORMS[(i + 1) % 2],) for i, c in enumerate(cases)]
    run_probes(batch, oracle_mod)


# ---------------------------------------------------------------------------------------------- B. the same edges through snf_edit_distance_batch_k
def check_k(items, oracle_mod):
    """items: [(A, B, k)], one call; k < 0: exact."""
    got = lib.edit_distance_batch([(a, b) for a, b, _ in items], max_dist=[k for _, _, k in items]).tolist()
    exp = [d if (k < 0 or d <= k) else -1 for d, k in ((dp(oracle_mod, a, b), k) for a, b, k in items)]
    wrong = [(i, len(items[i][0]), len(items[i][1]), items[i][2], e, g) for i, (e, g) in enumerate(zip(exp, got)) if e != g]
    assert wrong == [], f"(index, len A, len B, k, expected, got): {wrong[:8]}"


def hand_over_pairs():
    """m = 512 | 513, n - m = 0 | 1: the last pattern of the thread form and the first of the wave form."""
    rng = np.random.default_rng(24)
    out = []
    for m in (ee.THREAD_MAX, ee.THREAD_MAX + 1):
        for dl in (0, 1):
            for alphabet in (b"ACGT", b"ACGTN"):
                p = ee.rnd(rng, m, alphabet)
                out.append((p, ee.mutated(rng, p, 20, dl, alphabet)))
                out.append((ee.mutated(rng, p, 3, dl, alphabet), p))
    return out


def banded_items(pairs, oracle_mod):
    """check_banded's cut-offs (tests/test_edit_distance.py) for every pair: d - 1, d, d + 1, n - m - 1, 0, none."""
    out = []
    for a, b in pairs:
        d = dp(oracle_mod, a, b)
        out += [(a, b, k) for k in sorted({max(0, d - 1), d, d + 1, max(0, abs(len(a) - len(b)) - 1), 0, -1})]
    return out


@pytest.mark.parametrize("tier", TIERS)
def test_batch_k_short_edges(tier, oracle_mod):
    """The thread / wave hand-over, the shortcut's words and the rotating band through the tested entry point; the long pairs first, in
    the middle and last of the batch."""
    use_tier(tier)
    short = banded_items(hand_over_pairs() + [(a, b) for a, b, _ in ee.shortcut_pairs()], oracle_mod)
    rot = rotating_cases(oracle_mod)
    third = len(rot) // 3
    check_k(rot[:third] + short[:len(short) // 2] + rot[third:2 * third] + short[len(short) // 2:] + rot[2 * third:], oracle_mod)
    got = lib.edit_distance_batch([(a, b) for a, b, _ in rot[::3]] + hand_over_pairs()).tolist()          # no cut-offs at all: the other entry point
    assert got == [dp(oracle_mod, a, b) for a, b, _ in rot[::3]] + [dp(oracle_mod, a, b) for a, b in hand_over_pairs()]


def batch_wide_items(ms, alphabet):
    long = [c for m in ms for c in ee.wide_cases(m, alphabet)]
    short = [ee.filler(i) for i in range(3)] + [(a, b, 1) for a, b, _ in ee.shortcut_pairs()[:6]]
    third = len(long) // 3
    return long[:third] + short[:4] + long[third:2 * third] + short[4:] + long[2 * third:]


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", sorted(ee.ALPHABETS))
def test_batch_k_band_fit_edge_gpu(alphabet, oracle_mod):
    """ed_batch's host copy of the band rule decides who gets carry bytes, ed_wave's device copy who uses them: k = 3902 .. 3905 around
    d by construction with 63, 64 and 65 blocks; long pairs first, last and in the middle."""
    use_tier("gpu")
    items = batch_wide_items([ee.ROT] + ee.WIDE_M, alphabet)
    check_k(items, oracle_mod)
    check_k([(a, b, -1) for a, b, _ in items[:3] + items[-3:]], oracle_mod)          # no cut-off: kk = m, wide beyond 63 blocks


@pytest.mark.parametrize("alphabet", sorted(ee.ALPHABETS))
def test_batch_k_band_fit_edge_host(alphabet, oracle_mod):
    use_tier("host")
    items = [c for c in ee.wide_cases(ee.WIDE_M[0], alphabet)
             if c[2] - (len(c[1]) - len(c[0])) in (ee.BAND_EDGE - 1, ee.BAND_EDGE) and dp(oracle_mod, c[0], c[1]) in (c[2], c[2] + 1)]
    assert len(items) == 8
    check_k(items[:4] + [ee.filler(1), (b"ACGT", b"AGT", 1)] + items[4:], oracle_mod)


# ---------------------------------------------------------------------------------------------- C. the second round of the grid-stride loops
@pytest.mark.gpu
def test_ed_wave_second_stride_round_gpu(oracle_mod):
    """More wave-form pairs than ed_wave has workgroups: pair i and pair i + grid are different pairs with different distances."""
    use_tier("gpu")
    rng = np.random.default_rng(25)
    grid, n_distinct = E["ed_wave_grid"], 31
    assert grid % n_distinct
    distinct = []
    for i in range(n_distinct):
        p = ee.rnd(rng, ee.THREAD_MAX + 1 + 6 * i, b"ACGT" if i % 3 else b"ACGTN")
        distinct.append((p, ee.mutated(rng, p, 4 + 2 * i, i % 4)))
    ds = [dp(oracle_mod, a, b) for a, b in distinct]
    assert len(set(ds)) > n_distinct // 2 and all(min(len(a), len(b)) > ee.THREAD_MAX for a, b in distinct)
    n = grid + sc.WAVE
    idx = np.arange(n) % n_distinct
    assert all(ds[idx[i]] != ds[idx[i + grid]] for i in range(n - grid))
    pairs = [distinct[i] for i in idx]
    assert lib.edit_distance_batch(pairs).tolist() == [ds[i] for i in idx]
    ks = [ds[i] - (j % 2) for j, i in enumerate(idx)]                                # at the distance, and one below it
    assert lib.edit_distance_batch(pairs, max_dist=ks).tolist() == [ds[i] if j % 2 == 0 else -1 for j, i in enumerate(idx)]


def tiled_probes(n, n_distinct, oracle_mod):
    """n probe problems from n_distinct packed ones, every struct with an out_group slice of its own in one array.
    Returns (ctypes array, out array, expected out array, number of candidates per distinct probe, keep-alive)."""
    pairs = [(a, b) for _, a, b in ee.short_pairs() if 0 < min(len(a), len(b)) <= 2 * ee.BLOCK + 1 and dp(oracle_mod, a, b) > 0][:n_distinct]
    assert len(pairs) == n_distinct
    keep, base, exp, ncand = [], [], [], []
    for i, (a, b) in enumerate(pairs):
        k = max(0, dp(oracle_mod, a, b) - (i // 2) % 2)                              # at the distance, or one below it
        q, _, yes, no = ee.probe(a, b, k, ee.FORMS[i % 2], keep)
        base.append(np.frombuffer(bytes(q), abi.COMBINE_PROBLEM_DTYPE)[0])
        exp.append(yes if dp(oracle_mod, a, b) <= k else no)
        ncand.append(len(yes))
    idx = np.arange(n) % n_distinct
    rec = np.array(base, abi.COMBINE_PROBLEM_DTYPE)[idx].copy()
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.asarray(ncand)[idx], out=off[1:])
    out = np.full(int(off[-1]), -1, np.int32)
    rec["out_group"] = out.ctypes.data + 4 * off[:-1].astype(np.uint64)
    expected = np.concatenate([np.asarray(exp[i], np.int32) for i in idx])
    keep += [rec, out]
    return (abi.snf_combine_problem_t * n).from_buffer(rec), out, expected, [exp[i] for i in idx], keep


@pytest.mark.gpu
def test_combine_wave_second_stride_round_gpu(oracle_mod):
    """More problems than combine_problem_wave has workgroups; problem p and problem p + grid are different probes, and every problem
    writes a slice of its own, so a late problem that is skipped or run as an early one shows."""
    use_tier("gpu")
    grid, n_distinct = E["combine_wave_grid"], 61
    n = grid + sc.WAVE
    arr, out, expected, exp_by_problem, keep = tiled_probes(n, n_distinct, oracle_mod)
    assert grid % n_distinct and all(exp_by_problem[p] != exp_by_problem[p + grid] for p in range(n - grid))
    assert len({tuple(e) for e in exp_by_problem}) == 4                              # both forms, joined and not
    assert isinstance(arr, C.Array)
    lib.combine_resolve_batch(PROBE_CFG, arr)
    assert np.array_equal(out, expected), np.flatnonzero(out != expected)[:8]
    assert lib.combine_last_stats()["alignments"] == n


# ---------------------------------------------------------------------------------------------- D. the thread form of the merge on the GPU
@pytest.mark.gpu
def test_combine_thread_form_probes_gpu(oracle_mod, monkeypatch):
    """SNF_COMBINE_THREAD=1: combine_problem with ed_serial_k on the per-problem scratch e_off - the short, shortcut and multi-pass
    probes give what the wave form and the oracle give."""
    use_tier("gpu")
    cases = [(a, b, k, form) for _, a, b in ee.short_pairs() for k in ee.short_ks(a, b, dp(oracle_mod, a, b)) for form in ee.FORMS]
    cases += [(a, b, k, form) for a, b, d in ee.shortcut_pairs() for k in ((0,) if d == 0 else (0, 1)) for form in ee.FORMS]
    cases += interleaved(ee.wide_cases(ee.WIDE_M[0]), "group") + interleaved(ee.wide_cases(ee.WIDE_M[1], "planes")[::3], "pair")
    wave = run_probes(cases, oracle_mod, replay=False)
    assert lib.combine_last_stats()["dp_cells"] == sum(len(a) * len(b) for a, b, _, _ in cases)
    monkeypatch.setenv("SNF_COMBINE_THREAD", "1")
    assert run_probes(cases, oracle_mod) == wave


@pytest.mark.gpu
def test_combine_thread_form_batch_fuzz_vs_oracle_gpu(oracle_mod, monkeypatch):
    """The problems of test_combine.py::test_gpu_combine_batch_fuzz_vs_oracle in the thread form."""
    import copy

    import test_combine as tc
    from sniffles_amd import cluster
    use_tier("gpu")
    rng = np.random.default_rng(6)
    cfg = SnifflesConfig()
    problems = [(t, tc.random_problem(rng, t, int(rng.integers(1, 60))), []) for t in ["INS", "DEL", "DUP", "INV", "BND"] * 40]
    exp = [tc.oracle_resolve(oracle_mod)(t, c, copy.deepcopy(g), cfg) for t, c, g in problems]
    key = lambda gs: [([c.id for c in g.candidates], g.pos_mean, g.len_mean, g.bnd_mate_ref_start_mean) for g in gs]  # noqa: E731
    wave = cluster.resolve_block_groups_batch(copy.deepcopy(problems), cfg)
    n_aligned = lib.combine_last_stats()["alignments"]
    monkeypatch.setenv("SNF_COMBINE_THREAD", "1")
    got = cluster.resolve_block_groups_batch(problems, cfg)
    assert [key(g) for g in got] == [key(g) for g in exp] == [key(g) for g in wave]
    assert lib.combine_last_stats()["alignments"] == n_aligned > 0
