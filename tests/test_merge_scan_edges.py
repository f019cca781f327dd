"""Directed cases for the adaptive merge scan (snf_stage_cluster.h, stages B and C: compute_metrics, b1_seedmetrics_body, merge_criterion,
merge_walk, c1_mergeruns, c2_validate, c3_serial), which every cluster of every pass goes through.

The builders are in tests/merge_scan_cases.py, the restatement of cluster.py:48-61 / 219-308 they are planned on in tests/merge_scan_ref.py,
the literals come from size_classes.merge_thresholds().  Every case is checked four ways, all with `==`:
(a) the comparisons and merges it was written for occur in the restatement's trace (a case that has left its edge fails as such);
(b) Batch.fetch_clusters(0) and (1) are the restatement's clusters: start, end, repeat, n_leads_long, lead rows in list order;
(c) two run_pass calls and then call_candidates / finalize on one handle give the C oracle's candidates and final records, bit for bit;
(d) the handle's `[SNF_PROF] merge scan` line reports the planned number of runs, the resolved run_gap and - where the case plans it -
    the number of (task, svtype) groups redone serially.
Each case has a host-tier form and a `-m gpu` form, under the default pass and under SNF_CHAIN=0, SNF_NO_WINFRONT=1, SNF_NO_FUSE=1 and
SNF_MERGE_REREAD=1; the run-cut cases also under SNF_RUN_GAP unset / 0 / 100 / -1.  tests/golden/merge_scan_edges.json.gz holds the
unmodified reference's clusters for every table (oracle/make_golden.py::main_merge_scan_edges)."""
import json
import re

import numpy as np
import pytest

import golden_util as gu
import merge_scan_cases as mc
import merge_scan_ref as ref
import size_classes as sc
from sniffles_amd import lib, records, synth
from sniffles_amd.config import SnifflesConfig
from test_size_classes import prof, same_as_oracle, use_tier

T = sc.merge_thresholds()
FORMS = dict(default={}, chain0=dict(SNF_CHAIN="0"), nowinfront=dict(SNF_NO_WINFRONT="1"), nofuse=dict(SNF_NO_FUSE="1"), reread=dict(SNF_MERGE_REREAD="1"))
LINE = re.compile(r"\[SNF_PROF\] merge scan: (\d+) runs, (\d+) groups redone serially \(run_gap (-?\d+)\)$")


# ---------------------------------------------------------------------------------------------- the literals
def test_merge_literals_are_found_and_related():
    for k, v in T.items():
        assert isinstance(v, int) and v > 0, k
    assert T["sample_cap"] == sc.REF_METRICS == ref.MAX_N and T["added_below"] == 2 * T["sample_cap"]
    assert (T["added_below"] - 1) * ((1 << T["wide_shift"]) - 1) ** 2 < 1 << T["fits_shift"]
    assert mc.default_run_gap(SnifflesConfig()) == T["run_gap_floor"] == 1000
    assert mc.default_run_gap(SnifflesConfig(cluster_merge_bnd=5000)) == 5000 and mc.default_run_gap(SnifflesConfig(cluster_repeat_h_max=3e9)) == T["run_gap_max"]


@pytest.mark.parametrize("name,old,new", [
    ("snf_stage_cluster.h", "int64_t n = len < 100 ? len : 100;", "int64_t n = len < 100 ? len : 101;"),            # one rule, two numbers
    ("snf_stage_cluster.h", "const int64_t nn_ = Lm < 100 ? Lm : 100;", "const int64_t nn_ = Lm < 128 ? Lm : 128;"),  # the added sums with a cap of their own
    ("snf_stage_cluster.h", "&& Lm < 200 &&", "&& Lm < 201 &&"),                                                      # 200 leads: step 2, the sums do not add up
    ("snf_stage_cluster.h", ">> 27;", ">> 28;"),                                                                      # 199 squares of 2^28 pass 2^62
    ("snf_stage_cluster.h", "S1m > -((i128)1 << 62)", "S1m > -((i128)1 << 63)"),                                      # the bound written twice
    ("snf_stage_cluster.h", "constexpr int MCH = 32;", "constexpr int MCH = kBatch;"),                                # a literal no longer found
    ("snf_stage_cluster.h", "if (hd.n > 8)", "if (hd.n > 9)"),                                                        # nine leads in a group of eight
    ("snf_lib.hip", "(gap_base > 1000 ? gap_base : 1000)", "(gap_base > 1000 ? gap_base : 100)"),                     # the floor written twice
    ("snf_lib.hip", "gap_int(b->cfg.cluster_repeat_h_max) ? b->cfg.cluster_merge_bnd", "(int)b->cfg.cluster_repeat_h_max ? b->cfg.cluster_merge_bnd"),      # the cast unclamped
])
def test_a_broken_merge_literal_is_an_error(monkeypatch, name, old, new):
    real = sc._src
    assert old in real(name)
    monkeypatch.setattr(sc, "_src", lambda n: real(n).replace(old, new) if n == name else real(n))
    with pytest.raises(AssertionError):
        sc.merge_thresholds()


# ---------------------------------------------------------------------------------------------- the restatement against the reference
DOC = gu.load("merge_scan_edges")


def reference_rows(doc_case):
    return [tuple(tuple(x) if isinstance(x, list) else x for x in row) for row in doc_case["clusters"]]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_restatement_gives_the_reference_clusters(name):
    """The clusters the merge scan of the unmodified reference's cluster.resolve leaves for the table (yielded under --dev-no-resplit), as
    recorded: the same tasks (input hashes), the same clusters from the restatement - and the case still sits on its edge."""
    c = mc.CASES[name]
    tis = mc.build(c)
    assert [gu.input_sha(ti) for ti in tis] == DOC[name]["input_sha"]
    rows, _ = mc.planned(c, tis)
    assert [r[:6] + (len(r[6]),) for r in rows] == reference_rows(DOC[name])
    assert mc.lead_order_sha(rows, tis) == DOC[name]["lead_order_sha"]


def test_every_case_has_a_fixture_and_no_fixture_is_left_over():
    assert sorted(DOC) == sorted(mc.CASES)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_restatement_against_the_reference_itself(name):
    """Where the unmodified reference is at hand (oracle/_ref): its cluster.resolve, run now, against the restatement and the fixture."""
    import make_golden
    import ref_harness
    if not ref_harness.reference_available():
        pytest.skip("the reference is not importable here")
    c = mc.CASES[name]
    assert json.loads(json.dumps(make_golden.merge_scan_edges_doc(c))) == DOC[name]


# ---------------------------------------------------------------------------------------------- the check
def scan_lines(capfd):
    out = []
    for ln in prof(capfd)["merge scan"]:
        m = LINE.search(ln)
        assert m, ln
        out.append(tuple(int(x) for x in m.groups()))
    return out


def check_case(tier, name, form, gap, oracle_mod, monkeypatch, capfd):
    c = mc.CASES[name]
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    for k, v in {**FORMS[form], **c["env"]}.items():
        monkeypatch.setenv(k, v)
    if gap is None:
        monkeypatch.delenv("SNF_RUN_GAP", raising=False)
    else:
        monkeypatch.setenv("SNF_RUN_GAP", gap)
    tis, cfg = mc.build(c), mc.config(c)
    rows, _ = mc.planned(c, tis)                                                          # (a)
    rows0, _ = ref.batch_clusters(tis, cfg, stage=0)
    run_gap, runs, groups = mc.runs_planned(tis, cfg, gap)
    exp, exp_cand = oracle_mod.run(cfg, tis, True), records.records(oracle_mod.run(cfg, tis, False), tis, "cand")

    def report(n):                                                                        # (d)
        lines = scan_lines(capfd)
        assert len(lines) == n, lines
        for got_runs, got_dirty, got_gap in lines:
            assert (got_runs, got_gap) == (runs, run_gap), (lines, runs, run_gap)
            if gap in c["plan"]:
                assert got_dirty == c["plan"][gap], (lines, c["plan"])
            assert got_dirty <= groups and (run_gap >= 0 or got_dirty == 0), (lines, groups)
    with lib.Batch(cfg, tis) as b:
        capfd.readouterr()
        for _ in range(2):                                                                # (c)
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
            report(1)
        b.call_candidates()
        assert records.records(b.fetch(0), tis, "cand") == exp_cand
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)
        report(2)
        assert ref.library_clusters(b.fetch_clusters(1)) == rows                          # (b)
        assert ref.library_clusters(b.fetch_clusters(0)) == rows0


def form_params():
    return [(n, f) for n in sorted(mc.CASES) for f in (mc.CASES[n]["forms"] or FORMS)]


def cut_params():
    return [(n, g) for n in mc.CUT_CASES for g in mc.GAPS]


@pytest.mark.parametrize("name,form", form_params())
def test_merge_scan_host(name, form, oracle_mod, monkeypatch, capfd):
    check_case("host", name, form, None, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", form_params())
def test_merge_scan_gpu(name, form, oracle_mod, monkeypatch, capfd):
    check_case("gpu", name, form, None, oracle_mod, monkeypatch, capfd)


@pytest.mark.parametrize("name,gap", cut_params())
def test_merge_scan_run_cuts_host(name, gap, oracle_mod, monkeypatch, capfd):
    check_case("host", name, "default", gap, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("name,gap", cut_params())
def test_merge_scan_run_cuts_gpu(name, gap, oracle_mod, monkeypatch, capfd):
    check_case("gpu", name, "default", gap, oracle_mod, monkeypatch, capfd)


@pytest.mark.parametrize("name,gap", [(n, g) for n in ("cut_first_state_stdev", "cut_two_dirty_one_clean", "index_merge_at_2_behind_a_run_of_3") for g in ("0", "100")])
@pytest.mark.parametrize("form", ["chain0", "nofuse", "reread"])
def test_merge_scan_run_cuts_in_the_other_forms_host(name, gap, form, oracle_mod, monkeypatch, capfd):
    check_case("host", name, form, gap, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("name,gap", [(n, g) for n in ("cut_first_state_stdev", "cut_two_dirty_one_clean", "index_merge_at_2_behind_a_run_of_3") for g in ("0", "100")])
@pytest.mark.parametrize("form", ["chain0", "nofuse", "reread"])
def test_merge_scan_run_cuts_in_the_other_forms_gpu(name, gap, form, oracle_mod, monkeypatch, capfd):
    check_case("gpu", name, form, gap, oracle_mod, monkeypatch, capfd)


# ---------------------------------------------------------------------------------------------- (h) the small space, whole
def check_space(tier, ids, gaps, oracle_mod, monkeypatch, capfd):
    """Five three-lead seeds with k in {1, 39, 40} and 1 / 2 / 3 bins between them, every combination a group of its own: the
    library's merged clusters against the restatement, group by group, and the records against the oracle."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    tis, cfg = mc.space_tasks(ids), SnifflesConfig()
    assert len(tis) < 1 << 16 and sum(ti.n_leads for ti in tis) == 15 * len(ids) < 400_000
    rows, _ = ref.batch_clusters(tis, cfg)
    exp = records.records(oracle_mod.run(cfg, tis, True), tis, "final")
    for gap in gaps:
        if gap is None:
            monkeypatch.delenv("SNF_RUN_GAP", raising=False)
        else:
            monkeypatch.setenv("SNF_RUN_GAP", gap)
        run_gap, runs, groups = mc.runs_planned(tis, cfg, gap)
        assert runs == len(ids) if gap is None else runs > len(ids)          # (the default cut falls between the groups of the space and nowhere else)
        with lib.Batch(cfg, tis) as b:
            capfd.readouterr()
            b.run_pass()
            assert records.records(b.fetch(1), tis, "final") == exp
            (got_runs, got_dirty, got_gap), = scan_lines(capfd)
            assert (got_runs, got_gap) == (runs, run_gap) and got_dirty <= groups
            assert (got_dirty > 0) == (gap == "0")          # (no group spans 1 000 bp between two seeds; many merge across inner = 100 and 200)
            got = ref.library_clusters(b.fetch_clusters(1))
        assert len(got) == len(rows)
        assert got == rows


def test_the_small_space_sampled_host(oracle_mod, monkeypatch, capfd):
    ids = sorted(int(x) for x in np.random.default_rng(2718).choice(mc.SPACE_N, 2000, replace=False))
    check_space("host", ids, (None, "0"), oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
def test_the_small_space_whole_gpu(oracle_mod, monkeypatch, capfd):
    check_space("gpu", list(range(mc.SPACE_N)), (None, "0"), oracle_mod, monkeypatch, capfd)


# ---------------------------------------------------------------------------------------------- the fuzz tables of the host test, on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gap", [None, "0", "150", "-1"])
def test_merge_scan_run_cuts_are_exact_gpu(gap, oracle_mod, monkeypatch):
    """tests/test_emu_parity.py::test_merge_scan_run_cuts_are_exact on the device (default forms of the pass): neighbouring runs walk
    concurrently there, which the host tier - one workgroup after the other - cannot show."""
    assert lib.device_count() >= 1
    if gap is None:
        monkeypatch.delenv("SNF_RUN_GAP", raising=False)
    else:
        monkeypatch.setenv("SNF_RUN_GAP", gap)
    for seed in range(6):
        tis = [synth.gen_fuzz(100 * seed + k, task_id=k) for k in range(3)]
        for kw in ({}, dict(repeat=True, mosaic=True)):
            cfg = SnifflesConfig(**kw)
            exp = records.records(oracle_mod.run(cfg, tis, True), tis, "final")
            with lib.Batch(cfg, tis) as b:
                b.call_candidates()
                b.finalize()
                got = records.records(b.fetch(1), tis, "final")
            assert got == exp
