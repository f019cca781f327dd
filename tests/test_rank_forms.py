"""Directed cases for the rank sorts of d2w_call / wave_lead_agg (snf_wave_call.h::wave_sort_sets) and of the output stage
(snf_stage_out.h::f3k_rank).

wave_sort_sets ranks up to four key sets of a cluster in one loop over LDS rows and changes its lane form with the cluster's lead
count: up to 16 leads the four quarters of the wave rank four sets at once, up to 32 the two halves rank two, above that a lead per
lane.  The ladders of tests/cases.py pin 8 / 9, 23..25, 31..33 and 63..65 leads with one lead per read and distinct values; here are
15 / 16 / 17, tied values (every key equal but for the lane, strictly descending, two values alternating, random with repeats), reads
with two leads in one refined cluster (the phase tally's "last lead of a read wins"), and the sorts of resolve_bnd.  f3k_rank gives a
workgroup 256 consecutive kept calls and stages the keys of their tasks through LDS: the batches of section 4 put a workgroup inside one
task, across task borders and across an empty task, with calls of several types at EQUAL positions (the tie rule: candidate order).

Every case is compared with the C oracle on every field, bit for bit, and asserts from the oracle's own result that the planned
clusters came out as planned.  Every case has a host-tier form (tests/emu: the same sources on the fibre stand-in, f3k_rank included)
and a `-m gpu` form."""
import functools

import numpy as np
import pytest

import cases
from sniffles_amd import abi, lib, records
from sniffles_amd.config import SnifflesConfig
from test_size_classes import run, same_as_oracle, use_tier

SIZES = (9, 15, 16, 17, 31, 32, 33, 63, 64)       # both sides of the lane forms' edges (16, 32) and the ends of the range d2w_call takes
GAP = 20_000


def _pos(c):
    return 50_000 + c * GAP + 10          # (a cluster's leads lie within 64 bp of it: one 100-bp bin)


def _reads(n_clusters, depth=200):
    L = 50_000 + (n_clusters + 1) * GAP
    return cases._reads(depth, 0, L) + cases._reads(30, 0, L // 2, 1) + cases._reads(20, L // 3, L, 2), L


def pattern(kind, n, rng):
    """Offsets (>= 0, < 64) of the n leads of a cluster, in lead order."""
    if kind == 0:
        return [0] * n                                      # every key equal but for the lane
    if kind == 1:
        return [n - 1 - i for i in range(n)]                # strictly descending: the sort reverses the lanes
    if kind == 2:
        return [2 * (i % 2) for i in range(n)]              # two values, counts within 3 of each other (median_modes takes the middle one)
    return [int(x) for x in rng.integers(0, 6, n)]          # random with repeats


# ---------------------------------------------------------------------------------------------- 1. key sets at the lane-form edges
PLAIN = ("DEL", "INS", "DUP", "INV")


@functools.lru_cache(maxsize=None)
def edge_tasks():
    """One task per svtype, a cluster per size; the value patterns cycle over the clusters, shifted by the type, so every size meets
    every pattern.  svlen and ref_start follow the same pattern (DEL: negative svlen)."""
    tis = []
    for k, svtype in enumerate(PLAIN):
        rng = np.random.default_rng([91, k])
        allele = cases._rng_seq(rng, 400 + 64)
        leads = []
        for c, n in enumerate(SIZES):
            off = pattern((c + k) % 4, n, rng)
            for i in range(n):
                svlen = 400 + off[i]
                d = dict(svtype=svtype, ref_start=_pos(c) + off[i], svlen=-svlen if svtype == "DEL" else svlen, read=f"{svtype[0]}{c}_{i}",
                         strand="+-"[i % 2])
                if svtype == "INS":
                    d["seq"] = cases._mutate(rng, allele[:svlen], 0.02)
                if svtype in ("DUP", "INV"):
                    d["source"] = "SPLIT_SUP"
                leads.append(d)
        reads, L = _reads(len(SIZES))
        tis.append(cases.mk_task(leads, reads, L, task_id=k, contig=f"chrE{k}"))
    return tis


def check_key_set_edges(tier, mosaic, oracle_mod, monkeypatch):
    use_tier(tier, monkeypatch)
    tis = edge_tasks()
    cfg = SnifflesConfig(mosaic=mosaic, consensus_max_reads_bin=2000)
    exp = oracle_mod.run(cfg, tis, True)
    for t in range(len(tis)):       # no case passes because a cluster was split, merged or filtered
        lo, hi = int(exp.task_call_off[t]), int(exp.task_call_off[t + 1])
        assert sorted(int(n) for n in exp.calls["n_leads"][lo:hi]) == sorted(SIZES), PLAIN[t]
    same_as_oracle(run(cfg, tis), exp, tis)


@pytest.mark.parametrize("mosaic", [False, True], ids=["germline", "mosaic"])
def test_key_sets_at_the_lane_form_edges_host(mosaic, oracle_mod, monkeypatch):
    check_key_set_edges("host", mosaic, oracle_mod, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("mosaic", [False, True], ids=["germline", "mosaic"])
def test_key_sets_at_the_lane_form_edges_gpu(mosaic, oracle_mod, monkeypatch):
    check_key_set_edges("gpu", mosaic, oracle_mod, monkeypatch)


# ---------------------------------------------------------------------------------------------- 2. reads with two leads, the phase tally
TWO_LEAD_TYPES = ("DUP", "INV")      # (the oracle keeps both leads of a read in one refined cluster for these: asserted below)


@functools.lru_cache(maxsize=None)
def phased_tasks():
    """The same sizes; in every cluster the reads 0, 2 and 4 carry two leads (the second one as the cluster's last leads, with another
    `hap` / `ps`: it decides).  Clusters by c % 4: a clear majority of hap 1 / set P; two phase sets tied in count (the larger value wins)
    with the haplotypes tied as well; unphased throughout; a split with unphased leads in between."""
    tis = []
    for k, svtype in enumerate(TWO_LEAD_TYPES):
        rng = np.random.default_rng([92, k])
        leads = []
        for c, n in enumerate(SIZES):
            twice = (0, 2, 4)
            n_reads = n - len(twice)
            off = pattern((c + k + 1) % 4, n, rng)

            def phase_of(i, last):
                if c % 4 == 0:
                    return (2, f"Q{c}") if last else (1, f"P{c}")
                if c % 4 == 1:      # read i ends as hap 1 + i % 2, set P / Q (its first lead of two says the opposite): an even number of reads ties both tallies
                    cls = i % 2 if (last or i not in twice) else 1 - i % 2
                    return (1 + cls, (f"P{c}", f"Q{c}")[cls])
                if c % 4 == 2:
                    return (0, "NULL")
                return ((1, f"P{c}") if i % 3 else (0, "NULL")) if not last else (2, f"P{c}")
            order = [(i, False) for i in range(n_reads)] + [(i, True) for i in twice]
            for j, (i, last) in enumerate(order):
                hap, ps = phase_of(i, int(last))
                leads.append(dict(svtype=svtype, ref_start=_pos(c) + off[j], svlen=700 + off[j], read=f"{svtype[0]}{c}_{i}", strand="+-"[i % 2],
                                  source="SPLIT_SUP", hap=hap, ps=ps, qry_start=1000 + 7 * j + (9000 if last else 0)))
        reads, L = _reads(len(SIZES))
        tis.append(cases.mk_task(leads, reads, L, task_id=k, contig=f"chrP{k}"))
    return tis


def check_two_leads_per_read(tier, oracle_mod, monkeypatch):
    use_tier(tier, monkeypatch)
    tis = phased_tasks()
    cfg = SnifflesConfig(phase=True)
    exp = oracle_mod.run(cfg, tis, True)
    recs = records.records(exp, tis, "final")
    for t in range(len(tis)):
        lo, hi = int(exp.task_call_off[t]), int(exp.task_call_off[t + 1])
        nl, sup = exp.calls["n_leads"][lo:hi], exp.calls["support"][lo:hi]
        assert sorted(int(n) for n in nl) == sorted(SIZES), TWO_LEAD_TYPES[t]
        assert all(int(s) == int(n) - 3 for n, s in zip(nl, sup))           # at least one call per size has support < n_leads: all have
        assert 2 * sum(r["phase"] is not None for r in recs[t]) >= len(recs[t]), [r["phase"] for r in recs[t]]
    same_as_oracle(run(cfg, tis), exp, tis)


def test_reads_with_two_leads_and_the_phase_tally_host(oracle_mod, monkeypatch):
    check_two_leads_per_read("host", oracle_mod, monkeypatch)


@pytest.mark.gpu
def test_reads_with_two_leads_and_the_phase_tally_gpu(oracle_mod, monkeypatch):
    check_two_leads_per_read("gpu", oracle_mod, monkeypatch)


# ---------------------------------------------------------------------------------------------- 3. BND
BND_SIZES = (9, 16, 17, 32, 33)


@functools.lru_cache(maxsize=None)
def bnd_task(tied):
    """BND clusters behind a leading DEL cluster (a task of BNDs only is the reference's UnboundLocalError), two mate contigs in every
    cluster: a clear majority on chr7 (`tied` False), or as many leads on chr2 as on chr7 (n even) / one more on chr2 (n odd) - with
    equal counts the smallest contig wins.  Mate positions repeat; two reads carry two leads each."""
    rng = np.random.default_rng([93, int(tied)])
    leads = [dict(svtype="DEL", ref_start=3000 + i % 3, svlen=-400, read=f"d{i}", strand="+-"[i % 2]) for i in range(6)]
    for c, n in enumerate(BND_SIZES):
        off = pattern(c % 4, n, rng)
        for i in range(n):
            minor = (i % 2 == 0) if tied else (i % 4 == 1)
            mate = ("chr2", 700_000 + 2 * (i % 3), True, False) if minor else ("chr7", 90_000 + 2 * (i % 4), i % 3 == 0, i % 5 == 0)
            leads.append(dict(svtype="BND", ref_start=_pos(c) + off[i], read=f"b{c}_{i if i < n - 2 else i - n + 2}", strand="+-"[i % 2], mate=mate))
    reads, L = _reads(len(BND_SIZES))
    return cases.mk_task(leads, reads, L, contig="chrB")


def check_bnd(tier, tied, oracle_mod, monkeypatch):
    use_tier(tier, monkeypatch)
    tis = [bnd_task(tied)]
    for mosaic in (False, True):
        cfg = SnifflesConfig(mosaic=mosaic, dev_no_resplit=True)
        exp = oracle_mod.run(cfg, tis, True)
        bnd = exp.calls["svtype"] == cases.SVT["BND"]
        got_n = sorted(int(n) for n in exp.calls["n_leads"][bnd])
        if tied:
            plan = sorted((n + 1) // 2 for n in BND_SIZES)               # chr2: leads 0, 2, 4 ...
        else:
            plan = sorted(n - len(range(1, n, 4)) for n in BND_SIZES)   # chr7: all but leads 1, 5, 9 ...
        assert got_n == plan and all(g < n for g, n in zip(got_n, sorted(BND_SIZES)))      # resolve_bnd narrowed every cluster
        assert len(set(int(m) for m in exp.calls["mate_contig"][bnd])) == 1
        same_as_oracle(run(cfg, tis), exp, tis)


@pytest.mark.parametrize("tied", [False, True], ids=["majority", "tied"])
def test_bnd_sorts_at_the_lane_form_edges_host(tied, oracle_mod, monkeypatch):
    check_bnd("host", tied, oracle_mod, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("tied", [False, True], ids=["majority", "tied"])
def test_bnd_sorts_at_the_lane_form_edges_gpu(tied, oracle_mod, monkeypatch):
    check_bnd("gpu", tied, oracle_mod, monkeypatch)


# ---------------------------------------------------------------------------------------------- 4. output rank
RANK_TYPES = ("DEL", "INS", "DUP", "INV")


def rank_task(n_calls, task_id):
    """`n_calls` clusters of four leads under ten reads, each one call that passes QC.  Candidates come by type, then by position: the four types share
    their positions (call k of every type has the same `pos`) and within a type... the positions ascend, so the candidate order
    (type-major) interleaves in position order and calls of different types tie at equal `pos`."""
    rng = np.random.default_rng([94, n_calls, task_id])
    allele = cases._rng_seq(rng, 120)
    leads = []
    per = -(-n_calls // len(RANK_TYPES))
    made = 0
    for k, svtype in enumerate(RANK_TYPES):
        for j in range(per):
            if made == n_calls:
                break
            made += 1
            p = 20_010 + 2_000 * j
            for i in range(4):
                d = dict(svtype=svtype, read=f"t{task_id}{svtype[0]}{j}_{i}", strand="+-"[i % 2])
                if svtype == "DEL":         # pos = ref_start + svlen: the same `pos` as the others
                    d.update(ref_start=p + 300, svlen=-300)
                elif svtype == "INS":
                    d.update(ref_start=p, svlen=120, seq=cases._mutate(rng, allele, 0.02))
                else:
                    d.update(ref_start=p, svlen=700 + 200 * k, source="SPLIT_SUP")
                leads.append(d)
    L = 40_000 + 2_000 * per
    return cases.mk_task(leads, cases._reads(10, 0, L), L, task_id=task_id, contig=f"chrR{task_id}")


@functools.lru_cache(maxsize=None)
def rank_batch(mid):
    return [rank_task(n, t) for t, n in enumerate((1, mid, 0, 1025))]


def oracle_execute(exp, cfg):
    """CallTask.execute's two statements ([s for s in svcalls if s.qc], sorted by pos - stable) over the oracle's finalized candidates."""
    keep = []
    for t in range(len(exp.task_status)):
        lo, hi = int(exp.task_call_off[t]), int(exp.task_call_off[t + 1])
        idx = np.arange(lo, hi)
        idx = idx[exp.calls["qc"][lo:hi] != 0]
        keep.append(idx[np.argsort(exp.calls["pos"][idx], kind="stable")])
    return keep


def check_output_rank(tier, mid, oracle_mod, monkeypatch):
    """Execute mode with sorting on: the whole block against the oracle's candidates filtered and sorted, record order included; the same
    batch in candidate mode is the oracle's result as it stands.  The host tier runs f3k_rank itself (the fused output stage is part of
    the fibre stand-in's launch sequence)."""
    use_tier(tier, monkeypatch)
    tis = rank_batch(mid)
    cfg = SnifflesConfig()
    assert cfg.sort
    exp = oracle_mod.run(cfg, tis, True)
    keep = oracle_execute(exp, cfg)
    assert [len(k) for k in keep] == [1, mid, 0, 1025]
    idx = np.concatenate(keep)
    pos = exp.calls["pos"][idx]
    big = keep[3]
    assert (np.diff(big) < 0).sum() > 200 and (np.diff(exp.calls["pos"][big]) == 0).sum() > 500      # candidate order is not position order; ties
    with lib.Batch(cfg, tis) as b:
        b.set_output(abi.OUT_EXECUTE)
        b.call_candidates(); b.finalize()
        got = b.fetch(1)
        assert got.task_call_off.tolist() == np.concatenate([[0], np.cumsum([len(k) for k in keep])]).tolist()
        assert np.array_equal(got.calls["pos"], pos)
        for f in got.calls.dtype.names:
            if f in ("rn_off", "alt_off"):          # (where a record's read names and ALT bytes lie: compared below by content)
                continue
            a, e = got.calls[f], exp.calls[f][idx]
            if f == "cluster_seed_index":           # -1: not provided (records.diff_results)
                e = np.where(a == -1, -1, e)
            assert np.array_equal(a, e, equal_nan=a.dtype.kind == "f"), f
        for k, i in enumerate(idx.tolist()):
            assert got.alt(k) == exp.alt(i) and got.rn(k).tolist() == exp.rn(i).tolist()
        b.set_output(abi.OUT_CANDIDATES)
        b.call_candidates(); b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)


@pytest.mark.parametrize("mid", [255, 256, 257])
def test_output_rank_across_task_borders_host(mid, oracle_mod, monkeypatch):
    check_output_rank("host", mid, oracle_mod, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("mid", [255, 256, 257])
def test_output_rank_across_task_borders_gpu(mid, oracle_mod, monkeypatch):
    check_output_rank("gpu", mid, oracle_mod, monkeypatch)
