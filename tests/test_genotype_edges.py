"""`genotype_sv` and the 251 x 251 likelihood table at their edges, through `lib.genotype_batch` (snf_genotype_batch / g1_genotype: the
device function of the finalize kernels over caller-supplied records) and `postprocessing.genotype_svs` (the object path of --reqc).

What is pinned: every entry of the table the reference can reach (0 <= support <= coverage <= 250, the denormal and the zero
likelihoods of its last rows among them); the half-even roundings (the means of the coverage lists, 0.75 x and 0.5 x support, the
normalisation to 250, rescale_support); `support > coverage`; the failure on a coverage of zero; the DUP exception at dev_min_dup_vaf; the
z-score exemption of long insertions; the hom-alt phase tail.  The expected values are those of tests/genotype_ref.py - plain Python,
checked here against the unmodified reference where it is present - and, for the directed families, the reference's own recorded results
(tests/golden/genotype_edges.json.gz).  Every comparison is exact, VAF bit for bit.  Host tier (tests/emu) and `-m gpu`."""
import functools

import numpy as np
import pytest

import genotype_ref as gr
import golden_util as gu
import size_classes as sc
from sniffles_amd import lib, postprocessing, sv
from sniffles_amd.config import SnifflesConfig

TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]
GT_N = sc.coverage_thresholds()["gt_n"]


def use_tier(tier, monkeypatch):
    if tier == "host":
        import emu.emu as E
        E.lib()
    else:
        assert lib.device_count() >= 1


def make_cfg(over):
    return gr.apply(SnifflesConfig(), over)


def check(records, over, expected=None):
    """One launch over `records`; every field of gr.FIELDS against `expected` (default: the restatement)."""
    if expected is None:
        cfg = gr.config(over)
        expected = [gr.genotype(r, cfg) for r in records]
    got = gr.array_fields(lib.genotype_batch(make_cfg(over), gr.to_array(records)))
    want = [gr.expected_fields(r, e) for r, e in zip(records, expected)]
    bad = [(r, g, w) for r, g, w in zip(records, got, want) if g != w]
    assert bad == [], (len(bad), bad[:3])
    return expected


@functools.lru_cache(maxsize=None)
def fixture():
    return gu.load("genotype_edges")


# ---------------------------------------------------------------------------------------------- the expected values themselves
def test_families_are_the_recorded_ones_and_the_restatement_equals_the_recording():
    doc = fixture()
    fams = gr.fixture_families()
    assert [f[0] for f in fams] == sorted(doc) == ["directed", "directed_mosaic", "phase"]
    assert [len(f[2]) for f in fams] == [4356, 623, 60]
    for name, over, records in fams:
        assert doc[name]["config"] == over and doc[name]["records"] == records
        assert [gr.genotype(r, gr.config(over)) for r in records] == doc[name]["expected"], name
    exp = doc["directed"]["expected"]
    assert sum(e["filter"] == "GT_FAILED" for e in exp) > 500 and sum(e["filter"] == "GT" for e in exp) > 500
    assert {tuple(e["gt"][:2]) for e in exp if e["gt"]} == {(0, 0), (0, 1), (1, 1)}


def test_restatement_equals_the_unmodified_reference():
    """The live check: the reference's own postprocessing.genotype_sv on stand-in calls of its SVCall class, over every family of this
    module - the whole table included - and every configuration."""
    import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("reference sources not present")
    ref = rh.load_reference()
    n = 0
    for over, records in all_families():
        got = gr.on_objects(records, over, ref.sv.SVCall, sv.new_call, ref.postprocessing.genotype_sv, lambda: rh.make_config(()))
        assert got == [gr.genotype(r, gr.config(over)) for r in records], over
        n += len(records)
    assert n > 45_000


def test_the_last_rows_of_the_table_underflow():
    """With the default error the hom-ref likelihood 0.05^s x 0.95^(c - s) is denormal from s = 237 on and 0.0 from s = 249 on: the rows
    where `q1 / q2 > 0` of likelihood_ratio decides, and they are among the compared ones."""
    assert GT_N == gr.NORMALIZATION_TARGET + 1
    tiny = 2.2250738585072014e-308
    q = lambda s, c: (0.05 ** s) * (0.95 ** (c - s))
    assert q(236, 236) >= tiny > q(237, 237) > 0.0 and q(248, 248) > 0.0 and q(249, 249) == q(250, 250) == 0.0
    recs = gr.table_records()
    assert len(recs) == GT_N * (GT_N + 1) // 2 == 31_626
    assert sum(r["support"] >= 237 for r in recs) == sum(251 - s for s in range(237, 251))
    e = gr.genotype(gr.rec("DEL", 250, (0, 250, 250, 250, 0)), gr.config())
    assert e["gt"] == [1, 1, 60, 0, 250] and e["filter"] == "GT"         # qz == 0.0: the ratio is "not > 0", z reads 0 and the call is filtered
    e = gr.genotype(gr.rec("DEL", 248, (0, 248, 248, 248, 0)), gr.config())
    assert e["gt"] == [1, 1, 60, 0, 248] and e["filter"] == "PASS"       # ... one denormal earlier it is not


# ---------------------------------------------------------------------------------------------- 1. the whole table
CONFIGS = [({}, 1), (dict(genotype_error=0.01), 7), (dict(genotype_error=0.2), 7), (dict(mosaic=True), 7)]


def all_families():
    out = [(over, gr.table_records(stride)) for over, stride in CONFIGS]
    out += [(over, records) for _, over, records in gr.fixture_families()]
    out += [(over, records) for over, records in config_edge_families()]
    return out


@pytest.mark.parametrize("over,stride", CONFIGS, ids=["default", "error_0.01", "error_0.2", "mosaic"])
@pytest.mark.parametrize("tier", TIERS)
def test_the_whole_table(tier, over, stride, monkeypatch):
    """Every (support, coverage) with 0 <= support <= coverage <= 250 as a DEL with cov = (., c, c, c, .), one launch (every 7th pair for the
    other configurations): filter, qc, genotype, GQ, DR, DV, VAF bit for bit.  coverage == 0: GT_FAILED, qc false, no genotype."""
    use_tier(tier, monkeypatch)
    recs = gr.table_records(stride)
    assert len(recs) == (31_626 if stride == 1 else (31_626 + 6) // 7)
    exp = check(recs, over)
    assert exp[0] == dict(filter="GT_FAILED", qc=False, gt=None, vaf=None, gt_phase=None, phase=None) and recs[0]["cov"][1:4] == [0, 0, 0]
    assert all(e["gt"] is not None for e in exp[1:])
    if not over:
        assert sum(e["filter"] == "GT" for e in exp) > 1000 and sum(e["gt"][2] == 60 for e in exp[1:]) > 1000


# ---------------------------------------------------------------------------------------------- 2. directed records
@pytest.mark.parametrize("name", ["directed", "directed_mosaic"])
@pytest.mark.parametrize("tier", TIERS)
def test_directed_records(tier, name, monkeypatch):
    """Types x supports (around 250, 500, past 65 535) x coverage tuples (all zero, zeros among values, means that tie at .5 above an even
    and an odd floor, 250 / 251, ~500, 65 535) x support_sa x svlen around long_ins_length x filter, against the reference's recording."""
    use_tier(tier, monkeypatch)
    doc = fixture()[name]
    assert len(doc["records"]) == (4356 if name == "directed" else 623)
    check(doc["records"], doc["config"], doc["expected"])
    if name != "directed":
        return
    # the ties are ties: 20.5 -> 20, 21.5 -> 22, and 0.75 x 6 = 4.5 -> 4, 0.5 x 5 = 2.5 -> 2, 0.5 x 7 = 3.5 -> 4
    by = {(r["svtype"], r["support"], tuple(r["cov"]), r["filter"], r["support_sa"]): e for r, e in zip(doc["records"], doc["expected"])}
    assert by[("DEL", 2, (20, 20, 0, 21, 21), "PASS", None)]["gt"][3:] == [18, 2] and by[("DEL", 2, (21, 21, 0, 22, 22), "PASS", None)]["gt"][3:] == [20, 2]
    assert by[("DUP", 6, (12, 13, 14, 15, 16), "PASS", None)]["gt"][3:] == [14 + 4 - 6, 6]
    assert by[("INV", 5, (12, 13, 14, 15, 16), "PASS", None)]["gt"][3:] == [14 + 2 - 5, 5] and by[("INV", 7, (12, 13, 14, 15, 16), "PASS", None)]["gt"][3:] == [14 + 4 - 7, 7]
    assert by[("DEL", 1000, (12, 13, 14, 15, 16), "PASS", 3)]["gt"][3:] == [0, 1000]                   # support > coverage
    assert by[("DEL", 5, (0, 30, 0, 31, 0), "PASS", 3)]["gt"][3:] == [round((33 + 3 + 34) / 3) - 5, 5]   # (SUPPORT_SA is added before the zeros are dropped)


# ---------------------------------------------------------------------------------------------- 3. configuration edges
def config_edge_families():
    ins = gr.large_ins_records()
    probe = gr.rec("DEL", 8, (0, 30, 30, 30, 0))
    z = gr.z_score(probe, gr.config())
    return [(dict(detect_large_ins=True), ins), (dict(detect_large_ins=False), ins), (dict(pass_only=True), ins + gr.directed_records()[::11]),
            (dict(genotype_min_z_score=z), [probe]), (dict(genotype_min_z_score=z + 1), [probe]),
            ({}, gr.dup_vaf_records(2, 12)), (dict(dev_min_dup_vaf=0.2), gr.dup_vaf_records(3, 15)), (dict(long_ins_length=300), ins + gr.directed_records()[::13])]


@pytest.mark.parametrize("tier", TIERS)
def test_configuration_edges(tier, monkeypatch):
    """detect_large_ins on and off over long insertions whose z-score is below the threshold; pass_only; genotype_min_z_score at the
    z-score of a record and one above it; DUPs whose allele fraction equals dev_min_dup_vaf exactly and lies just below it while hom-ref
    is the likeliest genotype (the 0/1 override); another long_ins_length."""
    use_tier(tier, monkeypatch)
    fams = config_edge_families()
    res = [check(records, over) for over, records in fams]
    n_ins = len(gr.large_ins_records())
    assert n_ins == 60 and [len(f[1]) for f in fams] == [60, 60, 60 + 396, 1, 1, 3, 3, 60 + 336]
    on, off, pass_only = res[0], res[1], res[2]
    exempt = [i for i in range(n_ins) if on[i]["filter"] == "PASS" and off[i]["filter"] == "GT"]
    assert len(exempt) >= 10 and all(fams[0][1][i]["svlen"] >= 2500 for i in exempt)
    assert any(off[i]["filter"] == "GT" and fams[0][1][i]["svlen"] == 2499 and on[i]["filter"] == "GT" for i in range(n_ins))
    assert sum(e["filter"] == "GT" and not e["qc"] for e in pass_only) >= 20 and all(e["qc"] for e in off if e["filter"] == "GT")
    assert res[3][0]["filter"] == "PASS" and res[4][0]["filter"] == "GT" and 0 < fams[3][0]["genotype_min_z_score"] < 60
    for k, (num, den) in ((5, (2, 12)), (6, (3, 15))):
        at, below, plain = res[k]
        assert at["vaf"] == gr.config(fams[k][0])["dev_min_dup_vaf"] == num / den and below["vaf"] == num / (den + 1)
        assert (at["gt"][:2], at["filter"], at["qc"]) == ([0, 1], "PASS", True)            # the override, and the z-score filter waived
        assert (below["gt"][:2], below["filter"]) == ([0, 0], "GT") and (plain["gt"][:2], plain["filter"]) == ([0, 0], "GT")


# ---------------------------------------------------------------------------------------------- 4. the hom-alt phase tail
@pytest.mark.parametrize("tier", TIERS)
def test_the_hom_alt_phase_tail(tier, monkeypatch):
    """A call that genotypes to 1/1 keeps its haplotype although the phase filter failed (postprocessing.py:612-623), unless hp is 0; a
    0/1 call does not: ph_hp_pass, gt_hp, gt_ps."""
    use_tier(tier, monkeypatch)
    doc = fixture()["phase"]
    assert len(doc["records"]) == 60
    check(doc["records"], doc["config"], doc["expected"])
    rescued = [(r, e) for r, e in zip(doc["records"], doc["expected"]) if e["gt_phase"] is not None]
    assert len(rescued) == 3 * 2 * 2 and all(      # INS, DEL, BND (a DUP / INV of 30 reads in 30 is 0/1: support is added to the coverage)
        e["gt"][:2] == [1, 1] and r["phase"][0] != "0" and e["phase"][4] == "PASS" for r, e in rescued)
    assert any(e["gt"][:2] == [1, 1] and r["phase"][0] == "0" and e["gt_phase"] is None for r, e in zip(doc["records"], doc["expected"]))
    assert any(e["gt"][:2] == [0, 1] and r["phase"][0] == "1" and e["gt_phase"] is None and e["phase"][4] == "FAIL"
               for r, e in zip(doc["records"], doc["expected"]))


# ---------------------------------------------------------------------------------------------- 5. the object path
@pytest.mark.parametrize("tier", TIERS)
def test_the_object_path(tier, monkeypatch):
    """A tenth of the directed family and the phase family through postprocessing.genotype_svs on sv.SVCall objects: the phase tuple of
    the genotype, INFO PHASE and INFO VAF as the reference leaves them."""
    use_tier(tier, monkeypatch)
    doc = fixture()
    n = 0
    for name in ("directed", "phase"):
        records, expected = doc[name]["records"], doc[name]["expected"]
        if name == "directed":
            records, expected = records[::10], expected[::10]
        calls = []       # (the stand-in calls are collected, then genotyped in one launch)
        gr.on_objects(records, doc[name]["config"], sv.SVCall, sv.new_call, lambda c, cfg: calls.append((c, cfg)), SnifflesConfig)
        postprocessing.genotype_svs([c for c, _ in calls], calls[0][1])
        got = [gr.object_result(c) for c, _ in calls]
        assert got == expected, name
        n += len(records)
    assert n == 436 + 60
