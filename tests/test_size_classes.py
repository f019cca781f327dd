"""Directed cases at every size-class boundary of the kernels (tests/size_classes.py reads the boundaries from the sources).

Almost every stage of a pass picks a kernel form by size - clusters by lead count (d1g_refine<8> / d2g_call<8>: up to 8 leads, eight
clusters a wave; d1w_refine / d2w_call: up to 64, a lead per lane; x_big<0/1/2> beyond, with LDS rows up to SNF_BIG_STAGE_CAP /
SNF_BIG_FINAL_CAP leads), consensus calls by cons_class_of, the window front end by the largest window, e1w_finalize by SNF_E1_BATCH
calls per wave - and the forms change where kernels go wrong: the last lane, the last LDS row, the first item handed to the next
kernel.  The ladders of tests/cases.py put one cluster on either side of every boundary; their fixtures (tests/golden/ladder_*, from
the unmodified reference) are compared by test_oracle_golden.py, test_simt_tier.py and test_gpu_parity.py like every other case of
cases.ALL.  This module adds what those cannot: that the expected calls carry exactly the planned lead counts and the planned
consensus classes, the forms a handle reports, the batch shapes (calls per task, windows, passes over one handle), the consensus
class edges, and the kernel forms behind the library's switches.  Every comparison is bit-exact; every case has a host-tier form
(tests/emu) and a `-m gpu` form."""
import collections
import functools
import re

import numpy as np
import pytest

import cases
import golden_util as gu
import size_classes as sc
from sniffles_amd import lib, records
from sniffles_amd.config import SnifflesConfig

T = sc.thresholds()
PLAIN = ("INS", "DEL", "DUP", "INV", "BND")


def use_tier(tier, monkeypatch):
    """host: the product's sources on the fibre stand-in become the library of this test (and of sniffles_amd.consensus)."""
    if tier == "host":
        import emu.emu as E
        from sniffles_amd import consensus
        E.lib()
        monkeypatch.setattr(consensus._lib, "load", E.lib)
    else:
        assert lib.device_count() >= 1


def prof(capfd):
    """The [SNF_PROF] lines written since the last call, by their first words."""
    out = collections.defaultdict(list)
    for ln in capfd.readouterr().err.splitlines():
        m = re.match(r"\[SNF_PROF\] ([a-z A-Z]+?):", ln)
        if m:
            out[m.group(1)].append(ln)
    return out


def final(res, tis):
    return records.records(res, tis, "final")


def run(cfg, tis):
    with lib.Batch(cfg, tis) as b:
        b.call_candidates()
        b.finalize()
        return b.fetch(1)


def same_as_oracle(got, exp, tis):
    """Records (every field, ALT strings, supporting reads) and the coverage averages, bit for bit."""
    assert final(got, tis) == final(exp, tis)
    assert np.array_equal(got.coverage_average_total, exp.coverage_average_total, equal_nan=True)
    for t in range(len(tis)):
        assert records.diff_results(got, t, exp, t) == []


# ---------------------------------------------------------------------------------------------- 1. the thresholds themselves
def test_thresholds_are_found_and_the_ladders_straddle_them():
    for k, v in T.items():
        assert isinstance(v, int) and v > 0, k
    sizes = sc.ladder_sizes()
    for t in (sc.GROUP, T["heavy_n"], sc.HALF_WAVE, sc.WAVE, sc.TWO_WAVES, T["big_stage_cap"], sc.WIN_MID, T["big_final_cap"]):
        assert {t - 1, t, t + 1} <= set(sizes), t
    assert {sc.REF_METRICS, sc.REF_METRICS + 1} <= set(sizes)
    assert {T["win_maxcap"] - 1, T["win_maxcap"], T["win_maxcap"] + 1} <= set(sc.ladder_sizes(with_window_cap=True))
    assert sc.GROUP < T["heavy_n"] < sc.WAVE < T["big_stage_cap"] < T["big_final_cap"] < T["win_maxcap"]     # (SNF_HEAVY_N is honoured for 9..63)
    assert T["e1_batch"] == sc.WAVE


def test_a_missing_threshold_is_an_error(monkeypatch):
    monkeypatch.setattr(sc, "_src", lambda name: "// nothing here\n")
    with pytest.raises(AssertionError):
        sc.thresholds()


# ---------------------------------------------------------------------------------------------- 2. the ladders carry the planned sizes
def planned_n_leads(name):
    """len(cluster.leads) of every call a ladder case is built to give, ascending."""
    if name.startswith("ladder_refined_"):
        resplit, fuse = cases.refined_plan()
        out = [x for ab in resplit for x in ab]
        out += [6] if name.endswith("_bnd") else [n for n, _ in fuse]
    elif name.startswith("ladder_phased"):
        out = 2 * cases.phased_long_plan()
    elif name == "ladder_long_ins":
        out = list(cases.phased_long_plan())
    else:
        sizes, lead_in = cases.ladder_plan(name.split("_")[1].upper())
        out = list(sizes) + ([lead_in] if lead_in else [])
    return sorted(out)


@pytest.mark.parametrize("name", sorted(cases.LADDERS))
def test_ladder_fixtures_carry_the_planned_lead_counts(name, oracle_mod):
    """No ladder case passes because its clusters were filtered out, merged or split otherwise than planned: the calls of the oracle
    (equal to the reference's, test_oracle_golden.py) have exactly the planned multiset of lead counts at both stages, and the
    reference's own records - one read per lead in these cases - the same multiset of supporting reads."""
    build, kw, _ = cases.ALL[name]
    ti = build()
    doc = gu.load(name)
    assert gu.input_sha(ti) == doc["input_sha"]
    cfg = gu.make_config(kw, ti)
    plan = planned_n_leads(name)
    assert len(plan) >= 5 and max(plan) > sc.WAVE and min(plan) <= sc.WAVE
    for fin, key in ((False, "candidates"), (True, "final")):
        res = oracle_mod.run(cfg, [ti], fin)
        assert sorted(int(n) for n in res.calls["n_leads"]) == plan
        exp = doc["expected"][key]
        assert len(exp) == len(plan)
        if name != "ladder_long_ins":          # (there the supporting reads include those of leads_long)
            assert sorted(len(r["rnames"]) for r in exp) == plan
        else:
            assert sorted(len(r["rnames"]) for r in exp) == [n + 5 for n in plan]
            assert all(r["support_long"] == 7 for r in exp)
    if name.startswith("ladder_phased"):
        assert sum(r["phase"] is not None for r in doc["expected"]["final"]) >= len(plan) // 2
    if name.startswith("ladder_ins") or name == "ladder_long_ins":      # the consensus ran with n - 1 others and changed the best read
        assert sum(r["alt"] not in (None, "<INS>") for r in doc["expected"]["final"]) == len(plan)


# ---------------------------------------------------------------------------------------------- 2 + 5. the forms a handle launches
@functools.lru_cache(maxsize=None)
def plain_ladder_tasks():
    tis = []
    for k, svtype in enumerate(PLAIN):
        ti = cases.case_ladder(svtype)
        ti.task_id = k
        tis.append(ti)
    return tis


@functools.lru_cache(maxsize=None)
def plain_ladder_expected(mosaic):
    import oracle
    return oracle.run(SnifflesConfig(mosaic=mosaic), plain_ladder_tasks(), True)


# (environment, "path", grouped refine, grouped call) - the defaults first; the others are the forms the README's table lists and no
# other test selects: they are built into every library and have to give the same calls at every size class
FORMS = [
    ({}, "wave", "on", "on"),
    ({"SNF_NO_D1_GROUPS": "1"}, "wave", "off", "on"),
    ({"SNF_NO_D2_GROUPS": "1"}, "wave", "on", "off"),
    ({"SNF_D2_MID": "1"}, "wave", "on", "on"),
    ({"SNF_HEAVY_N": "9"}, "wave", "on", "on"),
    ({"SNF_HEAVY_N": "63"}, "wave", "on", "on"),
    ({"SNF_HEAVY_N": "0"}, "wave", "on", "on"),
    ({"SNF_NO_RN_DEFER": "1"}, "wave", "on", "on"),
    ({"SNF_NO_RN_FUSE": "1"}, "wave", "on", "on"),
    ({"SNF_NO_BIG_STAGE": "1"}, "wave", "on", "on"),
    ({"SNF_NO_WAVE": "1"}, "thread", "off", "off"),
]
FORM_IDS = ["-".join(f"{k}={v}" for k, v in f[0].items()) or "default" for f in FORMS]


def check_ladders_under(tier, form, oracle_mod, monkeypatch, capfd):
    """The five plain ladders in one batch, against the oracle.  On the wave path the thread bodies return at once for more than 64
    leads (snf_stage_call.h, snf_stage_final.h::e1_finalize_body): a correct call above 64 leads can only have come from x_big, one
    of at most 8 with grouped kernels on from d1g_refine / d2g_call - the handle's own report of its forms is asserted, not assumed."""
    env, path, d1g, d2g = form
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tis = plain_ladder_tasks()
    for mosaic in ((False, True) if not env else (False,)):
        capfd.readouterr()
        got = run(SnifflesConfig(mosaic=mosaic), tis)
        lines = prof(capfd)
        assert len(lines["forms"]) == 1, lines
        assert f"forms: {path} path," in lines["forms"][0] and f"grouped refine {d1g}, grouped call {d2g}" in lines["forms"][0], lines["forms"]
        exp = plain_ladder_expected(mosaic)
        for t, svtype in enumerate(PLAIN):      # the planned sizes came out of THIS library, each once
            lo, hi = int(got.task_call_off[t]), int(got.task_call_off[t + 1])
            assert sorted(int(n) for n in got.calls["n_leads"][lo:hi]) == planned_n_leads("ladder_" + svtype.lower()), svtype
        same_as_oracle(got, exp, tis)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_ladders_under_every_cluster_form_host(form, oracle_mod, monkeypatch, capfd):
    check_ladders_under("host", form, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_ladders_under_every_cluster_form_gpu(form, oracle_mod, monkeypatch, capfd):
    check_ladders_under("gpu", form, oracle_mod, monkeypatch, capfd)


def check_golden_ladder_forms(tier, name, monkeypatch, capfd):
    """Every ladder fixture (refined sizes, phased, long INS included) on the default forms: wave path, grouped refine and call on."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    build, kw, _ = cases.ALL[name]
    ti = build()
    doc = gu.load(name)
    capfd.readouterr()
    res = run(gu.make_config(kw, ti), [ti])
    lines = prof(capfd)
    assert len(lines["forms"]) == 1 and "forms: wave path," in lines["forms"][0] and "grouped refine on, grouped call on" in lines["forms"][0], lines["forms"]
    assert sorted(int(n) for n in res.calls["n_leads"]) == planned_n_leads(name)
    assert gu.diff_records(final(res, [ti])[0], doc["expected"]["final"]) == []
    assert float(res.coverage_average_total[0]) == doc["expected"]["coverage_average_total"]


LADDERS_NOT_PLAIN = sorted(n for n in cases.LADDERS if n.startswith(("ladder_refined", "ladder_phased", "ladder_long")))


@pytest.mark.parametrize("name", LADDERS_NOT_PLAIN)
def test_refined_phased_and_long_ladders_on_the_default_forms_host(name, monkeypatch, capfd):
    check_golden_ladder_forms("host", name, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LADDERS_NOT_PLAIN)
def test_refined_phased_and_long_ladders_on_the_default_forms_gpu(name, monkeypatch, capfd):
    check_golden_ladder_forms("gpu", name, monkeypatch, capfd)


# ---------------------------------------------------------------------------------------------- 3a. calls per task
def small_clusters_task(n_clusters, seed, task_id):
    """`n_clusters` clusters of 2..8 leads, 3 kb apart, the four types with a length and BND in turn (the first one never BND): each
    gives exactly one call.  n_clusters 0: a task with reads and no leads."""
    rng = np.random.default_rng([seed, 4001])
    allele = cases._rng_seq(rng, 90)
    leads = []
    for c in range(n_clusters):
        svtype = ("DEL", "INS", "DUP", "INV", "BND")[c % 5]
        for i in range(int(rng.integers(2, 9))):
            d = cases._ladder_lead(svtype, rng, 5_010 + 3_000 * c, f"t{task_id}c{c}_{i}", i, allele, c)
            leads.append(d)
    L = 20_000 + 3_000 * n_clusters
    return cases.mk_task(leads, cases._reads(30, 0, L) + cases._reads(9, 0, L // 2, 1), L, task_id=task_id, contig=f"chrC{task_id}")


CALL_COUNTS = sc.around(sc.GROUP) + sc.around(T["e1_batch"]) + sc.around(2 * T["e1_batch"])
CALL_BATCHES = [[n] for n in CALL_COUNTS] + \
    [[T["e1_batch"] - 1, 0], [0, T["e1_batch"]], [T["e1_batch"] + 1, 2 * T["e1_batch"] + 1], [2 * T["e1_batch"], sc.GROUP - 1]] + \
    [[63, 0, 64, 65, 0, 127, 128, 129, 8], [7, 8, 9, 0, 0, 64, 64, 65, 63], [0, 0, 0, 0, 0, 0, 0, 0, 65]]


def check_calls_per_task(tier, counts, oracle_mod, monkeypatch):
    """Tasks with exactly 64 k - 1, 64 k, 64 k + 1 calls (partial last waves of e1w_finalize) and 7 / 8 / 9 clusters in all (partial last
    groups of eight of d1g_refine / d2g_call), alone, in pairs and nine to a batch, empty tasks among them."""
    use_tier(tier, monkeypatch)
    tis = [small_clusters_task(n, 31 * k + n, k) for k, n in enumerate(counts)]
    for cfg in (SnifflesConfig(), SnifflesConfig(mosaic=True)):
        exp = oracle_mod.run(cfg, tis, True)
        assert [int(exp.task_call_off[t + 1] - exp.task_call_off[t]) for t in range(len(tis))] == list(counts)
        same_as_oracle(run(cfg, tis), exp, tis)


@pytest.mark.parametrize("counts", CALL_BATCHES, ids=lambda c: "+".join(map(str, c)))
def test_calls_per_task_at_the_batch_edges_host(counts, oracle_mod, monkeypatch):
    check_calls_per_task("host", counts, oracle_mod, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("counts", CALL_BATCHES, ids=lambda c: "+".join(map(str, c)))
def test_calls_per_task_at_the_batch_edges_gpu(counts, oracle_mod, monkeypatch):
    check_calls_per_task("gpu", counts, oracle_mod, monkeypatch)


# ---------------------------------------------------------------------------------------------- 3b. window edges
WINDOW_BP = 100 << 10      # the widest window the front end tries first: 2^10 bins of 100 bp (SNF_WIN_BITS_MAX default, cluster_binsize default)
MAX_WINS = sc.around(sc.WAVE)[1:] + sc.around(sc.WIN_MID)[1:] + sc.around(T["win_maxcap"])[1:]


def window_tasks(max_win, start):
    """A batch whose largest window holds exactly `max_win` leads at every width the front end tries: `max_win` DEL leads in ONE 100-bp
    bin.  Everything else lies in windows (of the widest kind) of their own, a handful of leads each.  `start`: where in its 64-position
    block of the bucket array the largest window begins - a wave of w4s_segment owns the windows that begin in its block, so its LDS rows
    reach 63 + CAP positions when the largest one begins at the block's last position (lone INS leads, which seed nothing, are put in
    front of it until it does; INS windows come before DEL windows, windows of a type in ascending order)."""
    rng = np.random.default_rng([max_win, 4003])
    allele = cases._rng_seq(rng, 90)
    big_win = 5
    leads = [cases._ladder_lead("DEL", rng, big_win * WINDOW_BP + 10, f"w{i}", i) for i in range(max_win)]
    before = 0
    for c, (svtype, win) in enumerate([("DEL", 0), ("DEL", 2), ("DEL", 8), ("INS", 5), ("DUP", 5), ("INV", 4), ("BND", 6), ("INS", 1)]):
        for i in range(3 + c):
            leads.append(cases._ladder_lead(svtype, rng, win * WINDOW_BP + 40_010 + 200 * c, f"s{c}_{i}", i, allele, c))
        if svtype == "INS" or (svtype == "DEL" and win < big_win):
            before += 3 + c
    for i in range((start - before) % 64):
        leads.append(dict(svtype="INS", ref_start=9 * WINDOW_BP + 1_010 + 300 * i, svlen=90, seq=allele, read=f"lone{i}"))
    L = 10 * WINDOW_BP
    t0 = cases.mk_task(leads, cases._reads(40, 0, L) + cases._reads(max_win // 2, 4 * WINDOW_BP, 7 * WINDOW_BP), L, task_id=0, contig="chrW")
    return [t0, small_clusters_task(9, max_win, 1)]


def check_window_edge(tier, max_win, start, oracle_mod, monkeypatch, capfd):
    """The window kernels come in instances for 64, 256 and SNF_WIN_MAXCAP leads, picked per batch from its largest window; above the
    largest instance the front end switches itself off and the sort path runs.  Three passes over one handle, then the two calls."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    tis = window_tasks(max_win, start)
    cfg = SnifflesConfig()
    exp = oracle_mod.run(cfg, tis, True)
    assert max(int(n) for n in exp.calls["n_leads"]) == max_win
    capfd.readouterr()
    with lib.Batch(cfg, tis) as b:
        lines = prof(capfd)["window front end"]
        assert len(lines) == 1, lines
        if max_win <= T["win_maxcap"]:
            assert "window front end: on " in lines[0] and f"largest {max_win} leads" in lines[0], lines
            assert f", {1 if max_win > sc.WAVE else 0} of more than 64:" in lines[0], lines
        else:
            assert "window front end: off " in lines[0], lines
        for _ in range(3):
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
        b.call_candidates(); b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)


@pytest.mark.parametrize("start", [0, 63])
@pytest.mark.parametrize("max_win", MAX_WINS)
def test_largest_window_at_the_instance_edges_host(max_win, start, oracle_mod, monkeypatch, capfd):
    check_window_edge("host", max_win, start, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [0, 63])
@pytest.mark.parametrize("max_win", MAX_WINS)
def test_largest_window_at_the_instance_edges_gpu(max_win, start, oracle_mod, monkeypatch, capfd):
    check_window_edge("gpu", max_win, start, oracle_mod, monkeypatch, capfd)


# ---------------------------------------------------------------------------------------------- 3c. passes over one ladder handle
def check_ladder_handle(tier, big, oracle_mod, monkeypatch):
    """A handle decides from the counts of its previous pass whether the next one launches x_big at all (hist_big): three passes, then
    call_candidates + finalize, over an input without a cluster above 64 leads (x_big is skipped from the second pass on) and over one
    with (it must be launched every time)."""
    use_tier(tier, monkeypatch)
    tis = []
    for k, svtype in enumerate(("DEL", "INS", "BND")):
        ti = cases.case_ladder(svtype, max_size=None if big else sc.WAVE)
        ti.task_id = k
        tis.append(ti)
    for cfg in (SnifflesConfig(), SnifflesConfig(mosaic=True, consensus_max_reads_bin=2000)):
        exp = oracle_mod.run(cfg, tis, True)
        top = max(int(n) for n in exp.calls["n_leads"])
        assert top == (T["win_maxcap"] + 1 if big else sc.WAVE)
        with lib.Batch(cfg, tis) as b:
            for _ in range(3):
                b.run_pass()
                same_as_oracle(b.fetch(1), exp, tis)
            b.call_candidates(); b.finalize()
            same_as_oracle(b.fetch(1), exp, tis)


@pytest.mark.parametrize("big", [False, True], ids=["at_most_64", "beyond_64"])
def test_passes_over_one_ladder_handle_host(big, oracle_mod, monkeypatch):
    check_ladder_handle("host", big, oracle_mod, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True], ids=["at_most_64", "beyond_64"])
def test_passes_over_one_ladder_handle_gpu(big, oracle_mod, monkeypatch):
    check_ladder_handle("gpu", big, oracle_mod, monkeypatch)


# ---------------------------------------------------------------------------------------------- 4. consensus class edges
def test_consensus_edge_table_matches_the_rule_in_the_sources():
    """The intended class of every problem equals cons_class_of as read from snf_stage_final.h, the problems sit ON the edges (the
    literal that decides is reached exactly on one side, exceeded by one on the other), and the reads are those the fixture was made from."""
    doc = gu.load("consensus_class_edges")
    probs = cases.consensus_edge_problems()
    assert [p["name"] for p in probs] == [d["name"] for d in doc["problems"]] == [e[0] for e in cases.CONS_EDGES]
    for p, d in zip(probs, doc["problems"]):
        assert cases.consensus_problem_sha(p) == d["input_sha"], p["name"]
        assert (len(p["best"]), len(p["others"]), p["skip"], p["klen"], p["cls"]) == (d["best_len"], d["n_others"], d["skip"], d["klen"], d["cls"])
        assert sc.cons_class(T, p["klen"], p["skip"], len(p["best"]), len(p["others"])) == p["cls"], p["name"]
    by = {p["name"]: p for p in probs}
    npos = lambda p: sc.cons_npos(len(p["best"]), p["klen"], p["skip"])
    assert npos(by["small_npos_120"]) == T["small_npos"] and npos(by["small_npos_121"]) == T["small_npos"] + 1
    assert len(by["small_len_384"]["best"]) == T["cons_small_l"] and len(by["small_len_385"]["best"]) == T["cons_small_l"] + 1
    assert len(by["small_others_64"]["others"]) == T["small_others"] and len(by["small_others_65"]["others"]) == T["small_others"] + 1
    assert by["small_skip_7"]["skip"] == T["small_skip"] and by["small_skip_8"]["skip"] == T["small_skip"] + 1
    assert npos(by["large_npos_500"]) == T["large_npos"] == T["rows_npos"] and npos(by["large_npos_501"]) == T["large_npos"] + 1
    assert len(by["large_others_254"]["others"]) == T["large_others"] and len(by["large_others_255"]["others"]) == T["large_others"] + 1
    assert len(by["large_len_8192"]["best"]) == T["cons_large_l"] and len(by["large_len_8193"]["best"]) == T["cons_large_l"] + 1
    assert len(by["rows_others_512"]["others"]) == T["rows_others"] and len(by["rows_others_513"]["others"]) == T["rows_others"] + 1
    assert len(by["rows_len_64999"]["best"]) == T["cons_l_end"] - 1 and len(by["rows_len_65000"]["best"]) == T["cons_l_end"]
    assert npos(by["rows_len_64999"]) == T["rows_npos"]
    assert by["klen_7"]["klen"] == T["cons_klen_max"] and by["klen_8"]["klen"] == T["cons_klen_max"] + 1
    for name in ("large_len_8193", "large_others_255", "rows_others_513", "large_npos_501", "rows_len_65000"):      # only ONE limit is passed
        p = by[name]
        assert npos(p) <= T["rows_npos"] + (name == "large_npos_501") and len(p["others"]) <= T["rows_others"] + (name == "rows_others_513")
    # at least a third of the expected strings differ from the best read (here: all of them - the best read carries errors of its own)
    assert 3 * sum(d["expected"] != p["best"] for p, d in zip(probs, doc["problems"])) >= len(probs)
    assert all(len(d["expected"]) == len(p["best"]) for p, d in zip(probs, doc["problems"]))


def check_consensus_edges_api(tier, monkeypatch):
    from sniffles_amd import consensus
    use_tier(tier, monkeypatch)
    doc = gu.load("consensus_class_edges")["problems"]
    probs = cases.consensus_edge_problems()
    by_klen = collections.defaultdict(list)
    for i, p in enumerate(probs):
        by_klen[p["klen"]].append(i)
    for klen, idx in sorted(by_klen.items()):       # one launch per k-mer length: every class and the thread kernels side by side
        got = consensus.novel_from_reads_batch([(probs[i]["best"], probs[i]["others"], probs[i]["skip"]) for i in idx], klen=klen)
        assert [probs[i]["name"] for i, g in zip(idx, got) if g != doc[i]["expected"]] == []
    for i in range(len(probs)):                     # ... and each problem alone (a kernel's first and only call)
        p = probs[i]
        got = consensus.novel_from_reads_batch([(p["best"], p["others"], p["skip"])], klen=p["klen"])
        assert got[0] == doc[i]["expected"], p["name"]


def test_consensus_class_edges_match_the_reference_host(monkeypatch):
    check_consensus_edges_api("host", monkeypatch)
    # the class each problem is GIVEN (the harness asks cons_class_of itself; it takes what the workgroup kernels take)
    from emu import simt
    doc = gu.load("consensus_class_edges")["problems"]
    probs = cases.consensus_edge_problems()
    for klen in sorted({p["klen"] for p in probs if p["cls"]}):
        idx = [i for i, p in enumerate(probs) if p["klen"] == klen and p["cls"]]
        got, cls, handed = simt.consensus_batch([(probs[i]["best"], probs[i]["others"], probs[i]["skip"]) for i in idx], klen)
        assert cls == [probs[i]["cls"] for i in idx]
        assert [probs[i]["name"] for i, g in zip(idx, got) if g != doc[i]["expected"]] == [] and handed == 0


@pytest.mark.gpu
def test_consensus_class_edges_match_the_reference_gpu(monkeypatch):
    check_consensus_edges_api("gpu", monkeypatch)


def consensus_pass_tasks(probs):
    """The problems as INS clusters of one task: best read and others as leads of equal svlen in one bin, each on its own read (any of them
    may be picked as the best read: the reads are all as long as the best one, so the class is the planned one whichever it is)."""
    rng = np.random.default_rng(4005)
    leads = []
    for c, p in enumerate(probs):
        for i, s in enumerate([p["best"]] + p["others"]):
            assert len(s) == len(p["best"])
            leads.append(dict(svtype="INS", ref_start=cases._ladder_pos(c) + int(rng.integers(0, 30)), svlen=len(s), seq=s,
                              read=f"c{c}_{i}", strand="+-"[i % 2]))
    reads, L = cases._ladder_reads(len(probs), depth=200)
    return [cases.mk_task(leads, reads, L)]


ALT_LISTS = re.compile(r"ALT lists copy (\d+) small (\d+) large (\d+)/(\d+)/(\d+)/(\d+) thread (\d+) rows (\d+)")


def check_consensus_edges_in_pass(tier, oracle_mod, monkeypatch, capfd):
    """The same edges inside whole passes: consensus_kmer_skip_base gives the sampling step (skip = base + int(L / 500)), one pass per
    (base, k-mer length); the populations of the pass's ALT lists are the planned number of calls per class."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    groups = collections.defaultdict(list)
    for p in cases.consensus_edge_problems(balanced=True):
        groups[(p["skip"] - int(len(p["best"]) * (1.0 / 500.0)), p["klen"])].append(p)
    assert len(groups) >= 8
    seen = collections.Counter()
    for (base, klen), probs in sorted(groups.items()):
        tis = consensus_pass_tasks(probs)
        cfg = SnifflesConfig(consensus_max_reads_bin=2000)
        cfg.consensus_kmer_skip_base, cfg.consensus_kmer_len = base, klen
        exp = oracle_mod.run(cfg, tis, True)
        assert sorted(int(n) for n in exp.calls["n_leads"]) == sorted(len(p["others"]) + 1 for p in probs)
        capfd.readouterr()
        got = run(cfg, tis)
        m = ALT_LISTS.search(prof(capfd)["counts"][-1])
        n = [int(x) for x in m.groups()]
        plan = collections.Counter(p["cls"] for p in probs)
        assert (n[0], n[1], sum(n[2:6]), n[6], n[7]) == (0, plan[1], plan[2], plan[0], plan[4]), ((base, klen), n, plan)
        seen.update(plan)
        same_as_oracle(got, exp, tis)
    assert seen == collections.Counter(e[5] for e in cases.CONS_EDGES) and min(seen[c] for c in (0, 1, 2, 4)) >= 4


def test_consensus_class_edges_inside_a_pass_host(oracle_mod, monkeypatch, capfd):
    check_consensus_edges_in_pass("host", oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
def test_consensus_class_edges_inside_a_pass_gpu(oracle_mod, monkeypatch, capfd):
    check_consensus_edges_in_pass("gpu", oracle_mod, monkeypatch, capfd)
