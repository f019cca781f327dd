"""Directed cases of `lib.population_match_batch` (snf_population_match_batch: `PopulationSNF.get_population_AF` for a batch of merged
calls) in both forms - one wave per query, and the thread form SNF_COMBINE_THREAD selects - against tests/popmatch_ref.py, a plain
restatement of snfp.py:91-155 over the exact DP of the C oracle.  All comparisons are exact.  The shapes are the smallest at which the
kernel can go wrong: list sizes around the wave width, the winner at the lane edges, more survivors of the positional gate than lanes,
ties, the edges of the two gates and of the alignment cut-off, the string shapes at which the alignment changes form, more queries
than the grid cap.  In every case the alignment counter lies between the queries answered by an insertion and the (query, insertion)
pairs that pass the positional gate: the kernel never aligns a pair the reference would not, and stops at the first accepted one.
`test_restatement_agrees_with_the_reference` holds the restatement itself against the unmodified reference on the same tables."""
import os
import re

import numpy as np
import pytest

import ed_edges as ee
import popmatch_ref as R
from popmatch_ref import V
from sniffles_amd import lib
from sniffles_amd.config import SnifflesConfig

TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]
FORMS = ("wave", "thread")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ref_cache = {}


def use_tier(tier):
    if tier == "host":
        import emu.emu as EM
        EM.lib()                                         # the host tier becomes the library of this test
    else:
        assert lib.device_count() >= 1


def s(b: bytes) -> str:
    return b.decode("latin-1")


def rnd(seed, n, alphabet=b"ACGT"):
    return s(ee.rnd(np.random.default_rng([31, seed, n]), n, alphabet))


def near(seed, a: str, edits: int) -> str:
    return s(ee.mutated(np.random.default_rng([32, seed]), a.encode("latin-1"), edits, 0))


def check(name, lists, queries, monkeypatch, oracle_mod, **options):
    """Both forms against the restatement (computed once per case and session); returns the wave form's stats."""
    cfg = SnifflesConfig(**options)
    if name not in _ref_cache:
        _ref_cache[name] = R.reference(lists, queries, cfg)
    want_best, want_dist, cnt = _ref_cache[name]
    table, q = R.pack(lists, queries)
    stats = {}
    for form in FORMS:
        if form == "thread":
            monkeypatch.setenv("SNF_COMBINE_THREAD", "1")
        else:
            monkeypatch.delenv("SNF_COMBINE_THREAD", raising=False)
        best, dist = lib.population_match_batch(cfg, table, q)
        st = stats[form] = lib.population_last_stats()
        assert np.array_equal(best, want_best), (name, form, np.flatnonzero(best != want_best)[:8])
        assert np.array_equal(dist, want_dist), (name, form, np.flatnonzero(dist != want_dist)[:8])
        assert cnt["ins_answers"] <= st["alignments"] <= cnt["gate_pairs"], (name, form, st, cnt)
    assert stats["wave"]["alignments"] == stats["thread"]["alignments"] and stats["wave"]["dp_cells"] == stats["thread"]["dp_cells"]
    monkeypatch.delenv("SNF_COMBINE_THREAD", raising=False)
    return stats["wave"], cnt, want_best


# ---------------------------------------------------------------------------------------------- list sizes
SIZES = [0, 1, 2, 63, 64, 65, 128, 129, 200]


def size_cases():
    """Per list size n an insertion list and a deletion list whose variants ALL pass the positional gate (dist = 1 + a permutation of
    0 .. n - 1: more than 64 survivors from n = 65 on).  Insertions: only the winner's ALT resembles the query's, so the search walks
    the survivors in dist order until it reaches it - the winner first, at index 63, at index 64 and last, at every rank of dist.
    Deletions have no sequence gate: the smallest dist wins."""
    lists, queries = [], []
    query_alt = rnd(1, 120)
    for n in SIZES:
        for winner in sorted({0, 63, 64, n - 1} & set(range(n))) or [None]:
            for rank in sorted({0, n // 2, n - 1} & set(range(n))) or [None]:
                order = np.random.default_rng([33, n]).permutation(n).tolist()
                if winner is not None:      # the winner is the rank-th nearest
                    order.remove(rank)
                    order.insert(winner, rank)
                lists.append([V(5000 + 1 + order[i], 120, near(i, query_alt, 3) if i == winner else rnd(100 + i, 120)) for i in range(n)])
                queries.append((V(5000, 120, query_alt), len(lists) - 1))
        lists.append([V(5000 - 1 - i if i % 2 else 5000 + 1 + i, -300, "<DEL>", "DEL") for i in np.random.default_rng([34, n]).permutation(n).tolist()])
        queries.append((V(5000, -300, "<DEL>", "DEL"), len(lists) - 1))
    queries.append((V(5000, 120, query_alt), -1))                       # no list at all
    queries.append((V(5000, -300, "<DEL>", "DEL"), -1))
    return lists, queries


@pytest.mark.parametrize("tier", TIERS)
def test_list_sizes_winner_positions_and_many_survivors(tier, monkeypatch, oracle_mod):
    use_tier(tier)
    lists, queries = size_cases()
    st, cnt, best = check("sizes", lists, queries, monkeypatch, oracle_mod)
    # every non-empty list has an answer, the empty ones and the queries without a list have none
    assert [int(b) >= 0 for b in best] == [li >= 0 and len(lists[li]) > 0 for _, li in queries]
    assert max(len(x) for x in lists) == 200 and st["alignments"] > cnt["ins_answers"]      # (survivors ahead of the winner were tried)


# ---------------------------------------------------------------------------------------------- ties and the order of the search
def tie_cases():
    a = rnd(2, 90)
    good, good2, bad = near(1, a, 2), near(2, a, 4), rnd(3, 90)
    q = V(7000, 90, a)
    lists = [
        [V(7010, 90, good), V(6990, 90, good2)],                        # equal dist, both accepted: the first
        [V(7010, 90, bad), V(6990, 90, good2)],                         # equal dist, the first fails the sequence gate
        [V(7005, 90, bad), V(7040, 90, good), V(7030, 90, good2)],      # the nearest fails, of the others the nearer one
        [V(7005, 90, bad), V(7005, 90, bad), V(6995, 90, bad)],         # all fail
        [V(7040, 90, good), V(7010, 90, good2), V(7010, 90, good)],     # a later variant is nearer; then equal dist: the first of them
        [V(7010, -90, "<DEL>", "DEL"), V(6990, -90, "<DEL>", "DEL"), V(7010, -90, "<DEL>", "DEL")],
    ]
    return lists, [(q if x[0].svtype == "INS" else V(7000, -90, "<DEL>", "DEL"), k) for k, x in enumerate(lists)]


@pytest.mark.parametrize("tier", TIERS)
def test_ties_and_sequence_gate_order(tier, monkeypatch, oracle_mod):
    use_tier(tier)
    lists, queries = tie_cases()
    st, cnt, best = check("ties", lists, queries, monkeypatch, oracle_mod)
    assert best.tolist() == [0, 3, 6, -1, 11, 13]
    assert st["alignments"] == 1 + 2 + 2 + 3 + 1                        # nothing behind the first accepted variant is aligned


# ---------------------------------------------------------------------------------------------- the positional gate
def gate_cases():
    """(name, options, lists, queries): deletions, so that the positional gate decides alone."""
    def d(pos, svlen):
        return V(pos, svlen, "<DEL>", "DEL")
    big = 4_000_000                                                     # sqrt(minlen) = 2000: only combine_match_max binds
    out = [("match_max", {}, [[d(5000 + 1000, -big)], [d(5000 + 1001, -big)], [d(5000 - 600, -big - 400)], [d(5000 - 600, -big + 401)]],
            [(d(5000, -big), k) for k in range(4)], [0, -1, 2, -1]),
           # minlen 16: 4 * combine_match exactly
           ("square", dict(combine_match=100), [[d(5400, 16)], [d(5401, 16)], [d(5000, 416)], [d(5000, 417)], [d(5399, 17)], [d(5400, 17)]],
            [(d(5000, 16), k) for k in range(6)], [0, -1, 2, -1, 4, -1]),
           # minlen 2: 250 * sqrt(2) = 353.55...
           ("non_square", {}, [[d(5353, 2)], [d(5354, 2)], [d(4647, -2)], [d(4646, -2)]], [(d(5000, 2), k) for k in range(4)], [0, -1, 2, -1]),
           # minlen 0: only dist 0 passes
           ("minlen0", {}, [[d(5000, 0)], [d(5001, 0)], [d(5000, 1)], [d(5000, 0)]], [(d(5000, 0), 0), (d(5000, 0), 1), (d(5000, 0), 2), (d(5000, 7), 3)],
            [0, -1, -1, -1]),
           # negative svlen on either side: the absolute values are compared
           ("signs", {}, [[d(5010, -200)], [d(5010, 200)], [d(5010, -200)], [d(5010, 230)]],
            [(d(5000, 200), 0), (d(5000, -200), 1), (d(5000, -230), 2), (d(5000, -200), 3)], [0, 1, 2, 3])]
    return out


@pytest.mark.parametrize("tier", TIERS)
def test_positional_gate_edges(tier, monkeypatch, oracle_mod):
    use_tier(tier)
    for name, options, lists, queries, expected in gate_cases():
        st, cnt, best = check("gate_" + name, lists, queries, monkeypatch, oracle_mod, **options)
        assert best.tolist() == expected, name
        assert st["alignments"] == 0


# ---------------------------------------------------------------------------------------------- the cut-off of the alignment
def cutoff_cases():
    lists, queries, expected = [], [], []

    def add(svlen, m, d, accepted, dl=0):
        a, b = ee.constructed(m, dl, d)
        lists.append([V(9000, svlen, s(a))])
        queries.append((V(9000, svlen, s(b)), len(lists) - 1))
        expected.append(accepted)
    add(10, 10, 2, True)            # (10 - 2) / 10 = 0.8 > 0.7
    add(10, 10, 3, False)           # (10 - 3) / 10 = 0.7 exactly: rejected; kmax = 2, d = kmax + 1
    add(20, 10, 5, True)            # svlen is the stored integer, not len(alt): (20 - 5) / 20 = 0.75
    add(20, 10, 6, False)           # (20 - 6) / 20 = 0.7
    add(100, 130, 29, True, dl=9)   # d = kmax
    add(100, 130, 30, False, dl=9)  # d = kmax + 1
    add(3, 40, 0, True)             # kmax = 0: identical strings only
    add(3, 40, 1, False)
    return lists, queries, expected


@pytest.mark.parametrize("tier", TIERS)
def test_cutoff_edges(tier, monkeypatch, oracle_mod):
    use_tier(tier)
    lists, queries, expected = cutoff_cases()
    st, cnt, best = check("cutoff", lists, queries, monkeypatch, oracle_mod)
    assert [int(b) >= 0 for b in best] == expected
    assert st["alignments"] == len(queries)
    # combine_pctseq = 0: no sequence gate, hence no alignment at all - everything passes
    st0, _, best0 = check("cutoff_pctseq0", lists, queries, monkeypatch, oracle_mod, combine_pctseq=0)
    assert st0["alignments"] == 0 and st0["dp_cells"] == 0 and (best0 >= 0).all()
    # an acceptance limit nothing can satisfy (kmax < 0): rejected without an alignment
    st1, _, best1 = check("cutoff_pctseq1", lists, queries, monkeypatch, oracle_mod, combine_pctseq=1.0)
    assert st1["alignments"] == 0 and (best1 < 0).all()


# ---------------------------------------------------------------------------------------------- string shapes
def shape_cases():
    lists, queries = [], []

    def add(valt, qalt, svlen=None):
        lists.append([V(3000, len(valt) if svlen is None else svlen, valt)])
        queries.append((V(3000, len(qalt) if svlen is None else svlen, qalt), len(lists) - 1))
    for n in (1, 8, 63, 64, 65, 512, 513):
        a = rnd(n, n)
        add(a, a)                                                       # identical
        add(a, near(n, a, max(1, n // 10)))                             # near
        add(a, near(n, a, max(1, n // 10)) + "ACGTACGT"[:1 + n % 7])    # near, other length
        add(a, rnd(1000 + n, n))                                        # unrelated
    seq = rnd(5, 200)
    add("<INS>", seq, svlen=200)                                        # a symbolic ALT against a sequence, both ways
    add(seq, "<INS>", svlen=200)
    add("<INS>", "<INS>", svlen=200)
    add(seq[:100] + "N" + seq[101:], seq)                               # an N in the variant's ALT (bit-plane form) / in the call's
    add(seq, seq[:50] + "N" + seq[51:])
    add(seq[:100] + "N" + seq[101:], seq[:100] + "N" + seq[101:])
    return lists, queries


@pytest.mark.parametrize("tier", TIERS)
def test_string_shapes(tier, monkeypatch, oracle_mod):
    use_tier(tier)
    lists, queries = shape_cases()
    st, cnt, best = check("shapes", lists, queries, monkeypatch, oracle_mod)
    assert 10 < int((best >= 0).sum()) < len(queries) and st["alignments"] == cnt["gate_pairs"] == len(queries)


def wide_cases():
    """Two queries with 7 000-byte ALTs at combine_pctseq 0.4: kmax = 4199, a band of 68 blocks for a pattern of 110 - it does not fit
    the wave (tests/size_classes.py::ed_band_is_wide) and takes the multi-pass form on the query's carry row; d = kmax and kmax + 1 by
    construction.  A short query in between has a carry row of eight bytes."""
    m, kmax = 7000, 4199
    assert ee.sc.ed_band_is_wide(ee.E, m, m, kmax) and m > ee.E["carry_min_len"]
    lists, queries = [], []
    for d in (kmax, 7, kmax + 1):
        a, b = ee.constructed(m if d > 100 else 50, 0, d)
        lists.append([V(100, len(a), s(a))])
        queries.append((V(100, len(b), s(b)), len(lists) - 1))
    return lists, queries


@pytest.mark.parametrize("tier", TIERS)
def test_cutoff_that_does_not_fit_the_band(tier, monkeypatch, oracle_mod):
    use_tier(tier)
    lists, queries = wide_cases()
    st, cnt, best = check("wide", lists, queries, monkeypatch, oracle_mod, combine_pctseq=0.4)
    assert best.tolist() == [0, 1, -1] and st["alignments"] == 3


# ---------------------------------------------------------------------------------------------- more queries than the grid
def grid_cap() -> int:
    with open(os.path.join(ROOT, "sniffles_amd", "csrc", "snf_combine.hip")) as f:
        m = re.findall(r"hipLaunchKernelGGL\(popmatch_wave, dim3\(\(unsigned\)\(nq < (\d+) \? nq : (\d+)\)\)", f.read())
    assert len(m) == 1 and m[0][0] == m[0][1], "the grid cap of popmatch_wave is no longer found in snf_combine.hip"
    return int(m[0][0])


@pytest.mark.gpu
def test_more_queries_than_the_grid_cap_gpu(monkeypatch, oracle_mod):
    """The second round of the stride loop of popmatch_wave: the tie and cut-off cases tiled to more queries than the cap.  The number
    of distinct queries does not divide the cap, so a wave's second query differs from its first."""
    use_tier("gpu")
    cap = grid_cap()
    l1, q1 = tie_cases()
    l2, q2, _ = cutoff_cases()
    lists = l1 + l2
    distinct = q1 + [(c, li + len(l1)) for c, li in q2]
    assert cap % len(distinct)
    n = cap + 3 * len(distinct) + 5
    want_best, want_dist, cnt = R.reference(lists, distinct, SnifflesConfig())
    reps = -(-n // len(distinct))
    queries = (distinct * reps)[:n]
    table, q = R.pack(lists, queries)
    for form in FORMS:
        if form == "thread":
            monkeypatch.setenv("SNF_COMBINE_THREAD", "1")
        best, dist = lib.population_match_batch(SnifflesConfig(), table, q)
        assert np.array_equal(best, np.tile(want_best, reps)[:n]) and np.array_equal(dist, np.tile(want_dist, reps)[:n]), form
        assert cnt["ins_answers"] * (reps - 1) <= lib.population_last_stats()["alignments"] <= cnt["gate_pairs"] * reps


# ---------------------------------------------------------------------------------------------- block keys (host side)
def _variant(contig, pos, svtype, svlen, alt, k):
    from sniffles_amd import snfp
    return snfp.PopulationVariant(contig=contig, pos=pos, id=f"v{k}", alt=alt, svtype=svtype, svlen=svlen, end=pos + abs(svlen), af=(k + 1) / 16 + 1e-7,
                                  genotyped_sample_count=k + 1, variant_sample_count=1)


def write_population(path, cfg, parts):
    """A population SNF with one part per entry of `parts`: (contig, [variants])."""
    from sniffles_amd import snf, snfp
    out = snfp.PopulationSNF(cfg, open(path, "wb"), filename=path)
    for task_id, (contig, variants) in enumerate(parts):
        name = f"{path}.tmp_{task_id}.snf"
        part = snfp.PopulationSNF(cfg, open(name, "wb"), filename=name)
        for v in variants:
            snf.SNFileBase.store(part, v)
        part.write_and_index()
        part.close()
        out.add_result(snf.SNFPart(task_id=task_id, contig=contig, snf_filename=name, snf_index=part.get_index(),
                                   snf_total_length=part.get_total_length(), snf_candidate_count=len(variants), coverage_average_total=0.0))
    cfg.snf_input_info = [dict(internal_id=k) for k in range(4)]
    out.write_results(cfg, sorted({c for c, _ in parts}))
    out.close()


@pytest.mark.parametrize("tier", TIERS)
def test_block_keys_and_first_part_only(tier, tmp_path):
    """A call's list is `blocks[contig][str(int(pos / block) * block)][svtype]`: calls at pos = block - 1, block and 0; a contig, a
    block and a type the file does not have.  Two tasks wrote into one block of chrB: only the first part is searched
    (`get_all_blocks` takes `read_blocks(...)[0]`, snf.py:231-239)."""
    from types import SimpleNamespace as NS
    from sniffles_amd import snfp
    use_tier(tier)
    cfg = SnifflesConfig()
    bs = cfg.snf_block_size
    parts = [("chrA", [_variant("chrA", bs - 1, "DEL", -100, "<DEL>", 0), _variant("chrA", bs, "DEL", -100, "<DEL>", 1),
                       _variant("chrA", 0, "DEL", -100, "<DEL>", 2), _variant("chrA", 3 * bs + 5, "INS", 60, "ACGT" * 15, 3)]),
             ("chrB", [_variant("chrB", 500, "DEL", -100, "<DEL>", 4)]),
             ("chrB", [_variant("chrB", 900, "DEL", -100, "<DEL>", 5), _variant("chrB", bs + 7, "DEL", -100, "<DEL>", 6)])]
    path = str(tmp_path / "pop.snf")
    write_population(path, cfg, parts)
    pop = snfp.PopulationSNF.open(path, cfg)
    assert pop.population == snfp.PopulationInfo(version=1, name="Population", description="A sample population", size=4)
    assert len(pop.index["chrB"]["0"]) == 2 and len(pop.index["chrB"][str(bs)]) == 1

    def call(contig, pos, svtype="DEL", svlen=-100, alt="<DEL>"):
        return NS(contig=contig, pos=pos, svtype=svtype, svlen=svlen, alt=alt)

    def answer(k):
        return (round((k + 1) / 16 + 1e-7, 5), k + 1)
    cases = [(call("chrA", bs - 1), answer(0)),          # the last position of block 0: the variant at bs is one base away, in another block
             (call("chrA", bs), answer(1)),
             (call("chrA", 0), answer(2)),
             (call("chrA", 1), answer(2)),
             (call("chrA", 3 * bs + 5, "INS", 60, "ACGT" * 15), answer(3)),
             (call("chrA", 3 * bs + 5, "INS", 60, "TTGCA" * 12), None),        # the sequence gate
             (call("chrA", 3 * bs + 5), None),           # a type the block does not have
             (call("chrA", 2 * bs + 5), None),           # a block the contig does not have
             (call("chrC", 0), None),                    # a contig the file does not have
             (call("chrA", 5, "BND", 0, "N[chr2:5["), None),
             (call("chrB", 500), answer(4)),
             (call("chrB", 900), answer(4)),             # v5 at 900 lies in the SECOND part of chrB's block 0: never searched - v4 (dist 400) it is
             (call("chrB", bs + 7), answer(6))]          # the first part of that block is the second task's
    af, size = pop.get_population_AF_batch([c for c, _ in cases])
    got = [None if a != a else (a, s) for a, s in zip(af.tolist(), size.tolist())]
    assert got == [w for _, w in cases]
    assert [pop.get_population_AF(c) for c, _ in cases] == [w for _, w in cases]
    assert [snfp.info_values(a, s) for a, s in zip(af.tolist(), size.tolist())][5] == (0, 0)
    assert all(isinstance(x, int) for x in snfp.info_values(float("nan"), 0))
    # an insertion the reference would divide by zero on: refused with the variant named, unless the sequence gate is off
    bad = str(tmp_path / "bad.snf")
    write_population(bad, cfg, [("chrA", [_variant("chrA", 10, "INS", 0, "ACGT", 0)])])
    with pytest.raises(ValueError, match="svlen 0"):
        snfp.PopulationSNF.open(bad, cfg).get_population_AF(call("chrA", 10, "INS", 4, "ACGT"))
    assert snfp.PopulationSNF.open(bad, SnifflesConfig(combine_pctseq=0)).get_population_AF(call("chrA", 10, "INS", 0, "ACGT")) == answer(0)


# ---------------------------------------------------------------------------------------------- the restatement against the reference
needs_ref = pytest.mark.skipif(not __import__("make_ref").ref_root(), reason="needs the reference (its checkout, or the staged build oracle/_ref that make_ref.py compiles)")


@needs_ref
def test_restatement_agrees_with_the_reference(oracle_mod):
    """tests/popmatch_ref.py against the UNMODIFIED `PopulationSNF.get_population_AF` (its `align` - edlib, absent here - patched to the
    same exact DP) on the tables of the directed cases: every list becomes block "0" of a contig of its own."""
    from types import SimpleNamespace as NS
    import ref_harness as rh
    rh.load_reference()
    from sniffles import snfp as ref_snfp
    keep = ref_snfp.align
    ref_snfp.align = lambda a, b, **kw: {"editDistance": oracle_mod.edit_distance(a.encode("latin-1"), b.encode("latin-1"))}
    try:
        runs = [("sizes", {}, *size_cases()), ("ties", {}, *tie_cases()), ("cutoff", {}, *cutoff_cases()[:2]),
                ("cutoff0", dict(combine_pctseq=0), *cutoff_cases()[:2]), ("shapes", {}, *shape_cases())]
        runs += [("gate_" + name, options, lists, queries) for name, options, lists, queries, _ in gate_cases()]
        for name, options, lists, queries in runs:
            cfg = rh.make_config(())                     # (SnifflesConfig.__init__ makes it SnifflesConfig.GLOBAL, config.py:619)
            for k, v in options.items():
                setattr(cfg, k, v)
            mine = SnifflesConfig(**options)
            assert (mine.combine_match, mine.combine_match_max, mine.combine_pctseq) == (cfg.combine_match, cfg.combine_match_max, cfg.combine_pctseq)
            psnf = ref_snfp.PopulationSNF(cfg, False)
            psnf._blocks["absent"] = {}
            gi = 0
            for li, variants in enumerate(lists):
                block = {}
                for v in variants:
                    block.setdefault(v.svtype, []).append(ref_snfp.PopulationVariant(
                        contig=f"c{li}", pos=v.pos, id=str(gi), alt=v.alt, svtype=v.svtype, svlen=v.svlen, end=0, af=0.5,
                        genotyped_sample_count=gi, variant_sample_count=1))
                    gi += 1
                psnf._blocks[f"c{li}"] = {"0": block}
            want = []
            for c, li in queries:
                assert 0 <= c.pos < cfg.snf_block_size
                r = psnf.get_population_AF(NS(contig=f"c{li}" if li >= 0 else "absent", pos=c.pos, svlen=c.svlen, svtype=c.svtype, alt=c.alt))
                want.append(-1 if r is None else r[1])
            best, _, _ = R.reference(lists, queries, mine)
            assert best.tolist() == want, name
    finally:
        ref_snfp.align = keep
