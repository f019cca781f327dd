"""The ALT consensus at its decision thresholds, in every form of the kernel.

consensus.novel_from_reads (consensus.py:280-394) takes eight kinds of decision - anchor shift, monotone chain, first anchor, clip at L,
segment identity, run filter, read filter, column vote - and every form of the kernel restates them: e45w_consensus SMALL (4 waves, 1
wave), LARGE (4 / 8 / 16 waves), ROWS, and the thread kernels e4_anchor / e5_align / e6_vote.  tests/consensus_cases.py places a problem
on either side of each threshold (and asserts from the trace of tests/consensus_ref.py that it sits there); this module runs the table
through every form: the class is moved without moving the decision by appending other reads that share no k-mer with the best read
(65 others: LARGE, 255: ROWS, 513: thread kernels), and asserted.  Expected strings: tests/golden/consensus_thresholds.json.gz, from the
unmodified reference.  Host tier (tests/emu) and `-m gpu`."""
import collections
import functools

import pytest

import consensus_cases as cc
import consensus_ref as cr
import golden_util as gu
import size_classes as sc
from test_consensus_api import _generic_problems, _wave_class_problems, needs_ref
from test_size_classes import use_tier

T = sc.thresholds()


@functools.lru_cache(maxsize=None)
def table():
    """[(case, expected string of the reference)]"""
    doc = gu.load("consensus_thresholds")["problems"]
    cs = cc.cases()
    assert [d["name"] for d in doc] == [c["name"] for c in cs]
    return [(c, d["expected"]) for c, d in zip(cs, doc)]


def planned_class(p):
    return sc.cons_class(T, p["klen"], p["skip"], len(p["best"]), len(p["others"]))


# ---------------------------------------------------------------------------------------------- the cases and the restatement
def test_integer_forms_decide_as_the_reference_float_quotients():
    """consensus_ref.py compares integers where the reference compares float quotients with 0.5, 0.2 and 0.25: the same decisions, over
    every pair the directed cases can meet (lengths up to 384, counts up to 600) and around the thresholds up to the kernels' limits."""
    for n in range(1, 601):
        for m in range(0, n + 1):
            q = m / float(n)
            assert (q >= 0.5) == (2 * m >= n) and (q > 0.5) == (2 * m > n) and (q > 0.2) == (5 * m > n) and (q < 0.25) == (4 * m < n), (m, n)
    for n in list(range(601, 65536, 97)) + list(range(65000, 65536)):
        for m in {n // 2 - 1, n // 2, n // 2 + 1, n // 5 - 1, n // 5, n // 5 + 1, n // 4 - 1, n // 4, n // 4 + 1}:
            q = m / float(n)
            assert (q >= 0.5) == (2 * m >= n) and (q > 0.5) == (2 * m > n) and (q > 0.2) == (5 * m > n) and (q < 0.25) == (4 * m < n), (m, n)


# a case on either side of every threshold whose outputs differ: (below / rejected, on or above / accepted)
SIDES = [
    ("seg_8_of_18", "seg_9_of_18"), ("seg_7_of_15", "seg_8_of_15"),                               # segment identity, even and odd n
    ("run_abs_5_of_8", "run_abs_6_of_8"), ("run_ratio_6_of_12", "run_ratio_7_of_12"),             # run filter, absolute and ratio
    ("span_24_of_120", "span_28_of_120"), ("span_24_of_120", "span_24_of_119"), ("span_28_of_140", "span_28_of_121"),   # read filter
    ("vote_4_of_maxal_17", "vote_4_of_maxal_16"), ("vote_margin_2_best_runner_up", "vote_margin_3_best_runner_up"),
    ("vote_margin_2_third_base_runner_up", "vote_margin_3_third_base_runner_up"), ("vote_lower_case_a_is_not_A", "vote_lower_case_a_loses_to_A"),
    ("first_anchor_j0_i_skip", "first_anchor_j_skip_i0"),
    ("shift_k6s3_j_ahead_9", "shift_k6s3_j_ahead_6"), ("shift_k6s3_i_ahead_9", "shift_k6s3_i_ahead_6"), ("shift_k7s3_j_ahead_9", "shift_k7s3_j_ahead_6"),
    ("shift_k4s1_j_ahead_5", "shift_k4s1_j_ahead_4"), ("shift_k4s1_i_ahead_5", "shift_k4s1_i_ahead_4"), ("shift_k4s4_j_ahead_8", "shift_k4s4_j_ahead_4"),
]


def test_cases_sit_on_their_edges_and_the_fixture_is_theirs():
    """Building the table asserts every `expect_trace` (consensus_cases._case).  Here: the fixture was recorded from these reads, the
    restatement gives the reference's string on every case, more than half of them change the best read, the two sides of every
    threshold give different columns, and appended unrelated reads change neither the string nor any decision of the other reads."""
    tab = table()
    doc = gu.load("consensus_thresholds")["problems"]
    for (c, exp), d in zip(tab, doc):
        assert cc.problem_sha(c) == d["input_sha"] and (c["klen"], c["skip"]) == (d["klen"], d["skip"]), c["name"]
        assert c["restated"] == exp, c["name"]
        assert [q for q in range(len(exp)) if exp[q] != c["best"][q]] == c["diff"], c["name"]
    assert 2 * sum(exp != c["best"] for c, exp in tab) >= len(tab)
    by = {c["name"]: c for c, _ in tab}
    for lo, hi in SIDES:
        assert by[lo]["diff"] == [] and by[hi]["diff"] != [], (lo, hi)
    assert all(planned_class(c) == 1 for c, _ in tab if len(c["others"]) <= 64)         # the base case is SMALL
    assert [planned_class(by[n]) for n in ("counter_254_votes_G", "counter_253_votes_G_and_1_A", "counter_255_votes_G")] == [2, 2, 4]
    for c, exp in tab:
        for n in cc.PADDINGS.values():
            p = cc.padded(c, n)
            if p is None:
                continue
            got, trace = cr.novel_from_reads(p["best"], p["others"], p["klen"], p["skip"])
            _, base = cr.novel_from_reads(c["best"], c["others"], c["klen"], c["skip"])
            pad = [("span", 0, len(c["best"]))] * (n - len(c["others"]))
            assert got == exp and [t for t in trace if t[0] != "vote"] == [t for t in base if t[0] != "vote"] + pad, (c["name"], n)
            assert [t for t in trace if t[0] == "vote"] == [t for t in base if t[0] == "vote"], (c["name"], n)    # maxal included


@needs_ref
def test_restatement_equals_the_reference():
    """String for string: the recorded vectors, both seeded generators of tests/test_consensus_api.py (gap bytes, skip_repetitive !=
    skip, indels, odd characters) and every directed case, plain, padded and with skip_repetitive 1."""
    import ref_harness as rh
    ref = rh.load_reference()

    class Lead:
        def __init__(self, seq):
            self.seq = seq
    probs = [(p["best"], p["others"], p["klen"], p["skip"], p["skip"]) for p in gu.load("consensus_novel_from_reads")["problems"]]
    assert len(probs) >= 160
    probs += [(p["best"], p["others"], p["klen"], p["skip"], p["skip_rep"]) for p in _generic_problems(17) + _wave_class_problems(29)]
    for c, _ in table():
        probs.append((c["best"], c["others"], c["klen"], c["skip"], c["skip"]))
        probs.append((c["best"], c["others"], c["klen"], c["skip"], 1))
        probs.append((c["best"], cc.padded(c, 300)["others"], c["klen"], c["skip"], c["skip"]))
    bad = []
    for k, (best, others, klen, skip, skip_rep) in enumerate(probs):
        exp = ref.consensus.novel_from_reads(Lead(best), [Lead(o) for o in others], klen, skip, skip_rep)
        if cr.novel_from_reads(best, others, klen, skip, skip_rep)[0] != exp:
            bad.append(k)
    assert bad == []
    for c, exp in table():
        assert ref.consensus.novel_from_reads(Lead(c["best"]), [Lead(o) for o in c["others"]], c["klen"], c["skip"], c["skip"]) == exp, c["name"]


# ---------------------------------------------------------------------------------------------- the table through the forms
def by_klen(problems):
    out = collections.defaultdict(list)
    for k, p in enumerate(problems):
        out[p["klen"]].append(k)
    return sorted(out.items())


def check_harness(problems, expected, want_cls, **form):
    """simt.consensus_batch: the product's workgroup kernels on the fibre stand-in, one launch per k-mer length; the class every
    problem RAN in is the harness's own report."""
    from emu import simt
    for klen, idx in by_klen(problems):
        got, cls, handed = simt.consensus_batch([(problems[k]["best"], problems[k]["others"], problems[k]["skip"]) for k in idx], klen, **form)
        assert cls == [want_cls(problems[k]) for k in idx]
        assert [problems[k]["name"] for k, g in zip(idx, got) if g != expected[k]] == []
        assert handed == 0      # (the two escape bytes of a case fit every escape list)


HOST_FORMS = [dict(), dict(mode=2), dict(mode=4), dict(nw=1), dict(nw=8), dict(mode=2, nw=8), dict(grid_cap=2), dict(nw=1, grid_cap=2)]


@pytest.mark.parametrize("form", HOST_FORMS, ids=lambda f: "-".join(f"{k}={v}" for k, v in f.items()) or "default")
def test_thresholds_in_the_workgroup_kernels_host(form):
    """SMALL with 4 waves and with 1, LARGE with 4 and 8 (mode 2 gives the SMALL problems to it), ROWS (mode 4), strided grids."""
    tab = table()
    mode = form.get("mode", 0)
    want = lambda p: 4 if mode == 4 else 2 if mode == 2 and planned_class(p) == 1 else planned_class(p)
    check_harness([c for c, _ in tab], [e for _, e in tab], want, **form)


@pytest.mark.parametrize("pad", ["large", "rows"])
def test_thresholds_padded_into_the_larger_classes_host(pad):
    """65 other reads: LARGE by n_others; 255: ROWS by n_others - the class the problems ran in is asserted."""
    n = cc.PADDINGS[pad]
    tab = [(cc.padded(c, n), e) for c, e in table() if cc.padded(c, n) is not None]
    assert len(tab) >= 70      # (all but the vote-counter cases, which have more other reads already)
    cls = {"large": 2, "rows": 4}[pad]
    assert all(planned_class(p) == cls for p, _ in tab)
    check_harness([p for p, _ in tab], [e for _, e in tab], lambda p: cls)


def skip_rep_1_cases():
    """(case, expected) with the best read's anchors sampled at every position (skip_repetitive = 1 != skip: the thread kernels) for the
    cases in which that changes no decision: the restatement's trace and string are those of skip_repetitive = skip."""
    out = []
    for c, exp in table():
        if c["skip"] == 1:
            continue
        got, trace = cr.novel_from_reads(c["best"], c["others"], c["klen"], c["skip"], 1)
        if (got, trace) == cr.novel_from_reads(c["best"], c["others"], c["klen"], c["skip"], c["skip"]) and got == exp:
            out.append((c, exp))
    assert 2 * len(out) >= len(table())
    return out


def check_api(tier, monkeypatch):
    """The library entry point: SMALL and LARGE with 4 waves, ROWS and the thread kernels (513 other reads; skip_repetitive != skip), all
    problems of one k-mer length in one launch, then every problem alone - a kernel's first and only call."""
    from sniffles_amd import consensus
    use_tier(tier, monkeypatch)
    probs, exp, rep = [], [], []
    for c, e in table():
        for n in (None,) + tuple(cc.PADDINGS.values()):
            p = c if n is None else cc.padded(c, n)
            if p is not None:
                assert n is None or planned_class(p) == {65: 2, 255: 4, 513: 0}[n]
                probs.append(p); exp.append(e); rep.append(p["skip"])
    for c, e in skip_rep_1_cases():
        probs.append(c); exp.append(e); rep.append(1)
    seen = collections.Counter(planned_class(p) if r == p["skip"] else 0 for p, r in zip(probs, rep))
    assert min(seen[k] for k in (0, 1, 2, 4)) >= 60, seen
    for klen, idx in by_klen(probs):
        got = consensus.novel_from_reads_batch([(probs[k]["best"], probs[k]["others"], probs[k]["skip"], rep[k]) for k in idx], klen=klen)
        assert [(probs[k]["name"], len(probs[k]["others"]), rep[k]) for k, g in zip(idx, got) if g != exp[k]] == []
    for k, p in enumerate(probs):
        if len(p["others"]) <= 255:
            assert consensus.novel_from_reads_batch([(p["best"], p["others"], p["skip"], rep[k])], klen=p["klen"])[0] == exp[k], (p["name"], len(p["others"]))


def test_thresholds_through_the_library_entry_point_host(monkeypatch):
    check_api("host", monkeypatch)


@pytest.mark.gpu
def test_thresholds_through_the_library_entry_point_gpu(monkeypatch):
    check_api("gpu", monkeypatch)


# ---------------------------------------------------------------------------------------------- inside whole passes
# The 1-wave SMALL instance (the default of a pass) and the 8- / 16-wave LARGE instances are launched by passes only.  A case becomes an
# INS cluster of one task: every read a lead of its own, all at ONE reference position and with svlen = its length, the best read first.
# annotate_sv (postprocessing.py:33-66) takes the first lead with the smallest |len(seq) - svlen| + 1.5 * |ref_start - pos|: all are
# equal, so the first lead of the cluster - the planned best read - is taken; that the plan holds is asserted on the C oracle's ALT.
# Left out, because they cannot be phrased as such a cluster: cases with other reads of another length than the best read (the two
# clip cases, the insertion in the middle, `other_reads_of_odd_lengths`), with fewer than two other reads or a best read below the INS length screen
# (`best_read_of_*`, `no_other_reads`, `one_other_read`, `vote_support_1`; `vote_support_2` only padded: below consensus_min_reads
# other reads the ALT is a verbatim copy), and `counter_255_votes_G` (ROWS has one form, reached above).
PASS_FORMS = [{}, {"SNF_CONS_NW": "4"}, {"SNF_CONS_LARGE_NW": "8"}, {"SNF_CONS_LARGE_NW": "16"}]


def cluster_cases():
    out = []
    for c, exp in table():
        if c["cluster"] and len(c["best"]) >= 60 and len(c["others"]) <= 254:
            if len(c["others"]) >= 4:       # (below consensus_min_reads the ALT is a verbatim copy)
                out.append((c, exp))
            if len(c["others"]) <= 64:
                out.append((cc.padded(c, cc.PADDINGS["large"]), exp))
    return out


def threshold_pass_task(probs):
    import cases
    leads = []
    for c, p in enumerate(probs):
        for i, s in enumerate([p["best"]] + p["others"]):
            assert len(s) == len(p["best"])
            leads.append(dict(svtype="INS", ref_start=cases._ladder_pos(c), svlen=len(s), seq=s, read=f"c{c}_{i}", strand="+-"[i % 2]))
    reads, L = cases._ladder_reads(len(probs), depth=200)
    return [cases.mk_task(leads, reads, L)]


def check_thresholds_in_pass(tier, env, oracle_mod, monkeypatch, capfd):
    import cases
    from sniffles_amd.config import SnifflesConfig
    from test_size_classes import ALT_LISTS, final, prof, run, same_as_oracle
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    groups = collections.defaultdict(list)
    for p, exp in cluster_cases():
        groups[(p["skip"], p["klen"])].append((p, exp))
    assert len(groups) >= 6 and sum(len(g) for g in groups.values()) >= 120
    for (skip, klen), grp in sorted(groups.items()):
        probs = [p for p, _ in grp]
        tis = threshold_pass_task(probs)
        cfg = SnifflesConfig(consensus_max_reads_bin=2000)
        cfg.consensus_kmer_skip_base, cfg.consensus_kmer_len = skip, klen      # (skip = base + int(L / 500) = base: L < 500)
        exp = oracle_mod.run(cfg, tis, True)
        recs = sorted(final(exp, tis)[0], key=lambda r: r["pos"])
        assert [r["pos"] for r in recs] == [cases._ladder_pos(c) for c in range(len(probs))]
        assert [p["name"] for (p, e), r in zip(grp, recs) if r["alt"] != e] == []      # the plan: the planned best read, the planned others
        capfd.readouterr()
        got = run(cfg, tis)
        n = [int(x) for x in ALT_LISTS.search(prof(capfd)["counts"][-1]).groups()]
        plan = collections.Counter(planned_class(p) for p in probs)
        assert (n[0], n[1], sum(n[2:6]), n[6], n[7]) == (0, plan[1], plan[2], 0, 0) and plan[1] + plan[2] == len(probs), ((skip, klen), n, plan)
        same_as_oracle(got, exp, tis)


@pytest.mark.parametrize("env", PASS_FORMS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_thresholds_inside_a_pass_host(env, oracle_mod, monkeypatch, capfd):
    check_thresholds_in_pass("host", env, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("env", PASS_FORMS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_thresholds_inside_a_pass_gpu(env, oracle_mod, monkeypatch, capfd):
    check_thresholds_in_pass("gpu", env, oracle_mod, monkeypatch, capfd)
