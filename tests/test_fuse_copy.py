"""merge_inner's fused sequences (cluster.py:85-122: curr_lead.seq += to_merge.seq) when the refine kernels only record the parts and
d1c_fusecopy moves the bytes on the side stream.

What can go wrong: a part copied short or long at an edge of the three copy forms (16 bytes per lane, a byte tail, 1-KB steps beyond
1 KB) or at an unaligned source / destination; a part recorded under the wrong slot, or not at all, at an edge of the lanes (a round of
four parts and one more, the group of eight of d1g_refine<8>, a whole wave, x_big<0> beside them); a part recorded although the fused
lead has no sequence; the ALT stage reading the pool before the copy has ended (the event edge, on every way into finalize); an entry
of an earlier pass or an earlier batch acted on again.  The fused bytes show as the ALT of an INS call whose best lead is a fused read:
verbatim with no_consensus (or fewer than consensus_min_reads other reads), through the consensus otherwise.

Every comparison is bit-exact against the C oracle; every case has a host-tier form (tests/emu) and a `-m gpu` form.  The host tier
runs streams in enqueue order, so a missing event edge cannot show there - that half is the GPU tier's."""
import functools

import numpy as np
import pytest

import cases
from sniffles_amd import cluster, lib, records
from sniffles_amd.config import SnifflesConfig

TIERS = [pytest.param("host", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
LARGE = {"SNF_CHAIN": "0", "SNF_GRAPH": "0"}      # the forms of a batch above the launch-bound size (what a whole genome runs)
IN_PLACE = {"SNF_FUSE_COPY": "0"}                  # the copies inside the refine kernels (the default of a handle that replays a graph)
SIDE = {"SNF_FUSE_COPY": "1"}                      # d1c_fusecopy also where passes are captured and replayed
NO_SLICES = {"SNF_NO_POOL_SLICES": "1"}
FORMS = [SIDE, LARGE, dict(SIDE, **NO_SLICES), dict(LARGE, **NO_SLICES), {}, dict(LARGE, **IN_PLACE)]
ids = lambda env: "-".join(f"{k}={v}" for k, v in env.items()) or "default"
PART_LENGTHS = (1, 15, 16, 17, 1023, 1024, 1025, 2049)
ALL_SEQ = dict(consensus_max_reads_bin=2000)      # no 10-per-bin cap: every lead keeps its sequence


def use_tier(tier, monkeypatch):
    if tier == "host":
        import emu.emu as E
        from sniffles_amd import consensus
        E.lib()
        monkeypatch.setattr(consensus._lib, "load", E.lib)
    else:
        assert lib.device_count() >= 1


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def final(res, tis):
    return records.records(res, tis, "final")


def same_as_oracle(got, exp, tis):
    assert final(got, tis) == final(exp, tis)
    for t in range(len(tis)):
        assert records.diff_results(got, t, exp, t) == []


# ---------------------------------------------------------------------------------------------- builder
def fuse_task(clusters, task_id=0, seed=0, distinct=(), step=20):
    """One INS cluster every 40 kb.  A cluster is a list of reads, a read a list of piece lengths (None: a piece without a sequence):
    the pieces of a read lie `step` bp apart on the reference and 40 bases apart on the read, so merge_inner fuses them in order
    (cluster_merge_pos = 150).  The first sequence of the pool is 3 bases long and every cluster's first piece comes behind whatever
    lengths precede it: sources and destinations are at no particular alignment.  distinct: the clusters in which every piece is a read
    of its own - the same leads and the same pool, and nothing fuses there."""
    rng = np.random.default_rng([seed, 7301, task_id])
    leads = [dict(svtype="INS", ref_start=2_000, svlen=3, read=f"t{task_id}pad", seq="ACG")]
    reads = []
    for c, cl in enumerate(clusters):
        pos = 20_010 + 40_000 * c
        width = max(len(r) for r in cl)
        allele = [cases._rng_seq(rng, max((r[k] or 0) for r in cl if len(r) > k) or 1) for k in range(width)]
        for r, pieces in enumerate(cl):
            q = 3_000 + 11 * r
            for k, plen in enumerate(pieces):
                n = 50 if plen is None else plen
                seq = None if plen is None else cases._mutate(rng, allele[k][:n], 0.02)
                name = f"t{task_id}c{c}r{r}" + (f"k{k}" if c in distinct else "")
                leads.append(dict(svtype="INS", ref_start=pos + step * k + (r % 3), svlen=n, read=name, qry_start=q, qry_end=q + n, seq=seq,
                                  strand="+-"[r % 2]))
                q += n + 40
        reads += [(pos - 5_000, pos + 8_000, 0)] * (len(cl) + 6)
    L = 60_000 + 40_000 * len(clusters)
    return cases.mk_task(leads, reads, L, task_id=task_id, contig=f"chrF{task_id}")


def lengths_clusters():
    # per length two clusters of six reads: an odd piece of 57 bases, then the length under test - and the other way round (a call needs
    # 50 bases; six reads: the consensus has its consensus_min_reads others)
    return [[pieces] * 6 for n in PART_LENGTHS for pieces in ([57, n], [n, 57])]


def counts_clusters():
    return [
        [[60, 61]] * 3,                                   # 2 parts
        [[50, 51, 52, 53]] * 2,                           # 4 parts: one round of four
        [[50, 51, 52, 53, 54]] * 2,                       # 5 parts: and one more
        [[51] * 8],                                       # 8 leads of one read: d1g_refine<8>
        [[52] * 9],                                       # 9 leads of one read: d1w_refine
        [[53] * 64],                                      # 64 leads of one read: one fused lead of 64 parts
        [[55, 56]] * 32,                                  # 32 reads with 2 parts each: 32 fused leads in one wave
        [[57] * 5] * 13,                                  # 65 leads: x_big<0> copies in place beside the others
    ]


def noseq_clusters():
    return [[[60, 61], [60, None], [60, 61], [None, 61, 62], [60, 61], [60, 61]]]


BATCHES = {
    "lengths": (lambda: (fuse_task(lengths_clusters(), 0, seed=1),), ALL_SEQ),
    "counts": (lambda: (fuse_task(counts_clusters(), 0, seed=2),), ALL_SEQ),
    "noseq": (lambda: (fuse_task(noseq_clusters(), 0, seed=3),), ALL_SEQ),
    # more than ten leads in a 100-bp bin (pieces 5 bp apart): the reference keeps ten sequences per bin, the rest are None
    "capped": (lambda: (fuse_task([[[45, 46, 47]] * 8], 0, seed=4, step=5),), {}),
    "two_tasks": (lambda: (fuse_task(counts_clusters()[:5], 0, seed=5), fuse_task(lengths_clusters()[6:10] + counts_clusters()[6:7], 1, seed=6)), ALL_SEQ),
    "unfused": (lambda: (fuse_task(counts_clusters()[:7], 0, seed=2, distinct=range(7)),), ALL_SEQ),
    # the same leads once more: fusions in the clusters at the back only / at the front only.  Their fused sequences are reserved from
    # the start of the same region, so an entry the first batch left behind lands on a fused sequence of the second
    "fused_back": (lambda: (fuse_task(counts_clusters()[:7], 0, seed=2, distinct=range(0, 4)),), ALL_SEQ),
    "fused_front": (lambda: (fuse_task(counts_clusters()[:7], 0, seed=2, distinct=range(4, 7)),), ALL_SEQ),
    "fused": (lambda: (fuse_task(counts_clusters()[:7], 0, seed=2),), ALL_SEQ),
}
CONFIGS = {"consensus": dict(minsupport=1), "verbatim": dict(minsupport=1, no_consensus=True)}


@functools.lru_cache(maxsize=None)
def expected(key, mode):
    """The oracle's result for a named batch and configuration, computed once and shared."""
    import oracle
    build, kw = BATCHES[key]
    cfg = SnifflesConfig(**dict(kw, **CONFIGS[mode]))
    tis = build()
    return tis, cfg, oracle.run(cfg, list(tis), True)


def ins_alts(exp, tis):
    return [c["alt"] for t in final(exp, list(tis)) if not isinstance(t, dict) for c in t if c["svtype"] == "INS" and c.get("alt")]


def run(cfg, tis):
    with lib.Batch(cfg, tis) as b:
        b.call_candidates()
        b.finalize()
        return b.fetch(1)


def check(tier, key, mode, env, monkeypatch):
    use_tier(tier, monkeypatch)
    set_env(monkeypatch, env)
    tis, cfg, exp = expected(key, mode)
    same_as_oracle(run(cfg, list(tis)), exp, list(tis))


# ---------------------------------------------------------------------------------------------- the batches are what they claim
def test_batches_carry_the_planned_fusions(oracle_mod):
    """The oracle's verbatim ALTs are the concatenations the builder planned: a fused read's pieces in order, every length under
    test, 64 parts in one lead, and leads without a sequence where a piece has none."""
    tis, cfg, exp = expected("lengths", "verbatim")
    assert sorted(len(a) for a in ins_alts(exp, tis)) == sorted(2 * [57 + n for n in PART_LENGTHS])
    tis, cfg, exp = expected("counts", "verbatim")
    assert sorted(len(a) for a in ins_alts(exp, tis)) == sorted([121, 206, 260, 8 * 51, 9 * 52, 64 * 53, 111, 5 * 57])
    tis, cfg, exp = expected("noseq", "verbatim")
    assert [len(a) for a in ins_alts(exp, tis)] == [121]
    tis, cfg, exp = expected("fused", "verbatim")
    assert max(len(a) for a in ins_alts(exp, tis)) == 64 * 53
    tis, cfg, exp = expected("unfused", "verbatim")      # the same leads, every piece a read of its own: the ALTs are input sequences
    assert len(ins_alts(exp, tis)) >= 7 and max(len(a) for a in ins_alts(exp, tis)) <= 61


def test_capped_bin_strips_sequences(oracle_mod):
    """24 leads in one 100-bp bin with consensus_max_reads_bin = 10: the leads beyond the tenth carry no sequence (leadprov.py:406-408),
    so fused leads of the batch have none; the consensus shows it - it differs from the one over all 24 sequences."""
    tis, cfg, exp = expected("capped", "consensus")
    assert int((tis[0].leads["seq_len"] >= 0).sum()) == 1 + 24      # the input has them all; the cap is the pipeline's
    uncapped = oracle_mod.run(SnifflesConfig(**dict(ALL_SEQ, **CONFIGS["consensus"])), list(tis), True)
    assert ins_alts(exp, tis) and ins_alts(exp, tis) != ins_alts(uncapped, tis)


# ---------------------------------------------------------------------------------------------- copy forms, lanes, reservations
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("mode", sorted(CONFIGS))
@pytest.mark.parametrize("form", FORMS, ids=ids)
@pytest.mark.parametrize("key", ["lengths", "counts"])
def test_part_lengths_and_counts_under_every_form(key, form, mode, tier, oracle_mod, monkeypatch):
    check(tier, key, mode, form, monkeypatch)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [SIDE, LARGE, IN_PLACE], ids=ids)
@pytest.mark.parametrize("key", ["noseq", "capped", "two_tasks"])
def test_parts_without_a_sequence_and_two_tasks(key, form, tier, oracle_mod, monkeypatch):
    for mode in sorted(CONFIGS):
        check(tier, key, mode, form, monkeypatch)


# ---------------------------------------------------------------------------------------------- pass after pass
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [SIDE, LARGE, dict(SIDE, **NO_SLICES), {}], ids=ids)
def test_four_passes_on_one_handle(form, tier, oracle_mod, monkeypatch):
    """run_pass four times: the second pass of a small batch is captured, the later ones replay the graph (SNF_FUSE_COPY=1: kernel and
    event edges inside it); every pass must find the table of parts as the first one did.  The default of such a handle is the
    in-place form; the large forms run every pass eagerly."""
    use_tier(tier, monkeypatch)
    set_env(monkeypatch, form)
    tis, cfg, exp = expected("counts", "verbatim")
    tis = list(tis)
    with lib.Batch(cfg, tis) as b:
        for _ in range(4):
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)


# ---------------------------------------------------------------------------------------------- the seams
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [SIDE, LARGE], ids=ids)
def test_every_way_into_finalize(form, tier, oracle_mod, monkeypatch):
    use_tier(tier, monkeypatch)
    set_env(monkeypatch, form)
    tis, cfg, exp = expected("counts", "consensus")
    tis = list(tis)
    with lib.Batch(cfg, tis) as b:      # two calls; finalize twice
        b.call_candidates()
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)
    with lib.Batch(cfg, tis) as b:      # a stage-0 fetch in between
        b.call_candidates()
        cand = b.fetch(0)
        assert len(cand.calls) == len(exp.calls)
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)
    with lib.Batch(cfg, tis) as b:      # the cluster fetch on fusing clusters: fused leads carry the sum of their parts' lengths
        b.call_candidates()
        cl = cluster.clusters_of(b, tis[0], 2)["INS"]
        assert {64 * 53, 9 * 52, 8 * 51, 111} <= {ld.svlen for c in cl for ld in c.leads}
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)
    with lib.Batch(cfg, tis) as b:      # the candidate stage twice before one finalize
        b.call_candidates()
        b.call_candidates()
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)


# ---------------------------------------------------------------------------------------------- an earlier batch's entries
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [SIDE, LARGE], ids=ids)
def test_the_next_batch_in_the_same_memory(form, tier, oracle_mod, monkeypatch):
    """A batch with many fusions, closed; its device memory goes to the slab cache and from there to a batch of the same size in which
    every piece is a read of its own: nothing fuses, and the ALTs are the input sequences.  Then the first batch once more, and two
    batches of the same leads that fuse in other clusters than their predecessor."""
    use_tier(tier, monkeypatch)
    set_env(monkeypatch, form)
    monkeypatch.delenv("SNF_NO_SLAB_CACHE", raising=False)
    for key in ("fused", "unfused", "fused", "fused_back", "fused_front", "fused_back"):
        tis, cfg, exp = expected(key, "verbatim")
        tis = list(tis)
        with lib.Batch(cfg, tis) as b:
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
