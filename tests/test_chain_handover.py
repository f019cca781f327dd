"""The middle of a pass - refine, refined-cluster table, call, compaction - with the hand-over lists built by the table kernels and
the tile sums of the two flag arrays published by whoever sets a flag.

Lists: c4_emit lists the merged clusters of more than 8 leads for d1w_refine, d1b_emit the refined clusters of more than 8 (with
SNF_D2_MID: 9..32 and more than 32) for the call kernels; the grouped kernels skip those items, and in an eager pass they run beside
the wave-per-item kernels.  A cluster that is on no list, or on a list and taken by the grouped kernel as well, is a missing or a
doubled call; the directed batches put clusters on both sides of every edge of the rule (8 / 9, heavy_n, 32 / 33, 64 / 65), leave a
list empty, leave the table walk without work, and let ONE merged cluster feed both call classes.

Sums: rc_emit counts a refined cluster into the 256-tile of its slot, the call kernels count a candidate into the tile of its refined
cluster; d1bk_rctable / d3ck_compact add up the tiles in front of their own.  A count that lands in the wrong tile, is made twice or
survives into the next pass shifts every later table entry: the batches put flags at the last slot of a tile and at the first of
the next, on both sides of 256 refined clusters, beyond the 64-tile edge of the former two-level sums, and run a handle over and
over.  Small batches take the single-launch chain forms and a captured pass by default; SNF_CHAIN=0 / SNF_GRAPH=0 select what a
large batch runs (two launches per chain, eager passes), which is where the published sums and the side-by-side launches are.

Every comparison is bit-exact against the C oracle; every case has a host-tier form (tests/emu) and a `-m gpu` form."""
import functools

import numpy as np
import pytest

import cases
import size_classes as sc
from sniffles_amd import lib, records
from sniffles_amd.config import SnifflesConfig

T = sc.thresholds()
LARGE = {"SNF_CHAIN": "0", "SNF_GRAPH": "0"}      # the forms of a batch above the launch-bound size
TIERS = [pytest.param("host", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


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


def run(cfg, tis):
    with lib.Batch(cfg, tis) as b:
        b.call_candidates()
        b.finalize()
        return b.fetch(1)


def same_as_oracle(got, exp, tis):
    assert final(got, tis) == final(exp, tis)
    assert np.array_equal(got.coverage_average_total, exp.coverage_average_total, equal_nan=True)
    for t in range(len(tis)):
        assert records.diff_results(got, t, exp, t) == []


def candidate_sizes(oracle_mod, cfg, tis):
    return sorted(int(n) for n in oracle_mod.run(cfg, tis, False).calls["n_leads"])


# ---------------------------------------------------------------------------------------------- builders
GAP = 3_000


def cluster_task(svtype, sizes, task_id=0, seed=0, lead_in=0, dropped=()):
    """One cluster of sizes[c] leads of `svtype` every 3 kb (each lead on a read of its own, all in one 100-bp bin: the occupancy
    prefilter keeps every lead, and cluster c occupies the L / F positions sum(sizes[:c]) ... of its task and type).  `dropped`:
    clusters whose DEL leads are 30 bp long - below minsvlen_screen, so call_from gives no candidate for them.  lead_in: a DEL
    cluster in front (a task of BNDs only is the reference's UnboundLocalError)."""
    rng = np.random.default_rng([seed, 4101, cases.SVT[svtype]])
    allele = cases._rng_seq(rng, 90)
    leads = [dict(svtype="DEL", ref_start=3_000 + i % 3, svlen=-400, read=f"t{task_id}d{i}", strand="+-"[i % 2]) for i in range(lead_in)]
    for c, n in enumerate(sizes):
        for i in range(n):
            d = cases._ladder_lead(svtype, rng, 5_010 + GAP * c, f"t{task_id}{svtype[0]}{c}_{i}", i, allele, c)
            if c in dropped:
                d["svlen"] = -30
            leads.append(d)
    L = 20_000 + GAP * len(sizes)
    return cases.mk_task(leads, cases._reads(30, 0, L) + cases._reads(9, 0, L // 2, 1), L, task_id=task_id, contig=f"chrH{task_id}")


def resplit_task(svtype, pairs, task_id=0, seed=0, before=()):
    """Merged clusters of a + b leads in two svlen modes (120 / 600) that resplit takes apart into refined clusters of a and of b leads,
    the first at the merged cluster's first F position, the second a positions further; `before`: whole clusters in front of them."""
    rng = np.random.default_rng([seed, 4102, cases.SVT[svtype]])
    alleles = (cases._rng_seq(rng, 120), cases._rng_seq(rng, 600))
    sign = -1 if svtype == "DEL" else 1
    leads = []
    for c, n in enumerate(before):
        leads += [cases._ladder_lead(svtype, rng, 5_010 + GAP * c, f"t{task_id}w{c}_{i}", i, alleles[0], c) for i in range(n)]
    for k, (a, b) in enumerate(pairs):
        c = len(before) + k
        for i in rng.permutation(a + b):
            big = int(i) >= a
            d = dict(svtype=svtype, ref_start=5_010 + GAP * c + int(rng.integers(0, 30)), svlen=sign * (600 if big else 120),
                     read=f"t{task_id}s{c}_{i}", strand="+-"[int(i) % 2])
            if svtype == "INS":
                d["seq"] = cases._mutate(rng, alleles[big], 0.03)
            leads.append(d)
    L = 20_000 + GAP * (len(before) + len(pairs))
    return cases.mk_task(leads, cases._reads(40, 0, L) + cases._reads(9, 0, L // 2, 1), L, task_id=task_id, contig=f"chrR{task_id}")


EDGES = sorted({sc.GROUP, sc.GROUP + 1, T["heavy_n"], T["heavy_n"] + 1, sc.HALF_WAVE, sc.HALF_WAVE + 1, sc.WAVE, sc.WAVE + 1})


@functools.lru_cache(maxsize=None)
def edge_tasks():
    return (cluster_task("DEL", EDGES, 0), cluster_task("INS", EDGES, 1), cluster_task("BND", EDGES, 2, lead_in=6),
            cluster_task("DUP", EDGES[::-1], 3))


@functools.lru_cache(maxsize=None)
def expected(key):
    """The oracle's result for a named batch, computed once and shared."""
    import oracle
    build, cfg = BATCHES[key]
    tis = build()
    return tis, cfg, oracle.run(cfg, list(tis), True)


BATCHES = {
    "edges": (edge_tasks, SnifflesConfig(consensus_max_reads_bin=2000)),
    "small_only": (lambda: (cluster_task("DEL", [2, 8, 3, 8, 5, 7, 8, 4, 6, 8, 8], 0), cluster_task("INS", [8, 2, 8], 1)), SnifflesConfig()),
    "large_only": (lambda: (cluster_task("DEL", [9, 40, 12, 25, 64, 33, 9, 10, 17], 0), cluster_task("INS", [9, 30], 1)),
                   SnifflesConfig(consensus_max_reads_bin=2000)),
    "empty_tasks": (lambda: (cluster_task("DEL", [], 0), cluster_task("DEL", [9, 3, 8, 20], 1), cluster_task("DEL", [], 2),
                             cluster_task("INS", [4, 12], 3), cluster_task("DEL", [], 4)), SnifflesConfig()),
    "empty_batch": (lambda: (cluster_task("DEL", [], 0), cluster_task("INS", [], 1)), SnifflesConfig()),
    # one merged cluster of 9..64 leads -> refined clusters on both sides of 8: the refine stage takes it in d1w_refine, the call stage
    # in d2g_call<8> AND d2w_call
    "resplit": (lambda: (resplit_task("DEL", [(5, 20), (3, 9), (8, 9), (30, 34), (2, 7)], 0), resplit_task("INS", [(4, 11), (20, 6)], 1)),
                SnifflesConfig(consensus_max_reads_bin=2000)),
    # 50 clusters of 5 leads, then a merged cluster whose two refined clusters start at F positions 250 and 255 - the last slot of the
    # first 256-tile -, then a cluster at 256, the first slot of the next
    "tile_edge_slots": (lambda: (resplit_task("DEL", [(5, 1), (4, 4)], 0, before=[5] * 50),), SnifflesConfig()),
}
for _k in (255, 256, 257):      # refined clusters: the last call flag at the last slot of tile 0, the first and the second of tile 1
    BATCHES[f"n_rc_{_k}"] = ((lambda k=_k: (cluster_task("DEL", [2] * k, 0, seed=k),)), SnifflesConfig())
# refined clusters 255 and 256 - a tile's last and the next tile's first slot - give no candidate
BATCHES["dropped_at_tile_edge"] = (lambda: (cluster_task("DEL", [2] * 260, 0, seed=9, dropped=(255, 256)),), SnifflesConfig())
# just over 16 384 kept lead positions: 65 tiles, one more than a super tile of the two-level sums held
BATCHES["beyond_64_tiles"] = (lambda: (cluster_task("DEL", [8, 9] * 965, 0, seed=11),), SnifflesConfig())


def check(tier, key, env, monkeypatch):
    use_tier(tier, monkeypatch)
    set_env(monkeypatch, env)
    tis, cfg, exp = expected(key)
    same_as_oracle(run(cfg, list(tis)), exp, list(tis))


# ---------------------------------------------------------------------------------------------- the batches are what they claim
def test_batches_carry_the_planned_clusters(oracle_mod):
    tis, cfg, _ = expected("edges")
    assert candidate_sizes(oracle_mod, cfg, list(tis)) == sorted(4 * EDGES + [6])
    assert {sc.GROUP, sc.GROUP + 1, T["heavy_n"], T["heavy_n"] + 1, 32, 33, 64, 65} == set(EDGES)
    tis, cfg, _ = expected("resplit")
    assert candidate_sizes(oracle_mod, cfg, list(tis)) == sorted([5, 20, 3, 9, 8, 9, 30, 34, 2, 7, 4, 11, 20, 6])
    tis, cfg, _ = expected("tile_edge_slots")
    assert candidate_sizes(oracle_mod, cfg, list(tis)) == sorted([5] * 50 + [5, 1, 4, 4])
    for k in (255, 256, 257):
        tis, cfg, _ = expected(f"n_rc_{k}")
        assert candidate_sizes(oracle_mod, cfg, list(tis)) == [2] * k
    tis, cfg, _ = expected("dropped_at_tile_edge")
    assert candidate_sizes(oracle_mod, cfg, list(tis)) == [2] * 258
    tis, cfg, _ = expected("beyond_64_tiles")
    assert sum(t.n_leads for t in tis) == 965 * 17 > 64 * 256 and candidate_sizes(oracle_mod, cfg, list(tis)) == sorted([8, 9] * 965)
    tis, cfg, exp = expected("empty_batch")
    assert sum(t.n_leads for t in tis) == 0 and len(exp.calls) == 0
    tis, cfg, _ = expected("small_only")
    assert max(candidate_sizes(oracle_mod, cfg, list(tis))) == sc.GROUP
    tis, cfg, _ = expected("large_only")
    assert min(candidate_sizes(oracle_mod, cfg, list(tis))) == sc.GROUP + 1


# ---------------------------------------------------------------------------------------------- lists from the table kernels
LIST_FORMS = [{}, {"SNF_D2_MID": "1"}, {"SNF_HEAVY_N": "0"}, {"SNF_HEAVY_N": "9"}, {"SNF_HEAVY_N": "63"}, {"SNF_NO_D1_GROUPS": "1"},
              {"SNF_NO_D2_GROUPS": "1"}]
ids = lambda env: "-".join(f"{k}={v}" for k, v in env.items()) or "default"


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("large", [False, True], ids=["small_forms", "large_forms"])
@pytest.mark.parametrize("form", LIST_FORMS, ids=ids)
def test_size_edges_under_every_list_form(form, large, tier, oracle_mod, monkeypatch):
    check(tier, "edges", dict(form, **(LARGE if large else {})), monkeypatch)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [{}, LARGE, dict(LARGE, SNF_D2_MID="1")], ids=["small_forms", "large_forms", "large_forms_mid"])
@pytest.mark.parametrize("key", ["small_only", "large_only", "empty_tasks", "empty_batch", "resplit"])
def test_lists_empty_full_and_fed_by_one_cluster(key, form, tier, oracle_mod, monkeypatch):
    check(tier, key, form, monkeypatch)


# ---------------------------------------------------------------------------------------------- published sums
SUM_KEYS = ["n_rc_255", "n_rc_256", "n_rc_257", "tile_edge_slots", "dropped_at_tile_edge", "beyond_64_tiles"]
SUM_FORMS = [LARGE, {"SNF_CHAIN": "1"}, dict(LARGE, SNF_NO_WAVE="1")]


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", SUM_FORMS, ids=["large_forms", "chain", "large_forms_no_wave"])
@pytest.mark.parametrize("key", SUM_KEYS)
def test_published_sums_at_the_tile_edges(key, form, tier, oracle_mod, monkeypatch):
    check(tier, key, form, monkeypatch)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [LARGE, {}], ids=["large_forms", "small_forms"])
@pytest.mark.parametrize("key", ["dropped_at_tile_edge", "resplit"])
def test_a_handle_gives_the_same_block_pass_after_pass(key, form, tier, oracle_mod, monkeypatch):
    """The rows of the published sums are zeroed by the pass itself: three passes on one handle, then call_candidates twice before one
    finalize (the second run of the candidate stage starts from the flags and sums the first one left)."""
    use_tier(tier, monkeypatch)
    set_env(monkeypatch, form)
    tis, cfg, exp = expected(key)
    tis = list(tis)
    with lib.Batch(cfg, tis) as b:
        for _ in range(3):
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
        b.call_candidates()
        b.call_candidates()
        b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)


# ---------------------------------------------------------------------------------------------- side by side: no order between the classes
@pytest.mark.parametrize("order", ["reverse", "random:1", "random:20261018"])
@pytest.mark.parametrize("key", ["edges", "resplit", "tile_edge_slots"])
def test_workgroup_and_lane_order_have_no_say_host(key, order, oracle_mod, monkeypatch):
    """The grouped and the wave-per-item kernel of a stage share no item and no output entry, and the tile sums are commutative: the
    host tier runs the lanes of a wave and the workgroups of a launch in descending / shuffled order."""
    monkeypatch.setenv("SNF_SIMT_ORDER", order)
    check("host", key, LARGE, monkeypatch)
