"""Directed cases of `lib.genotype_match_batch` (snf_genotype_match_batch: the match of `GenotypeTask.execute`, reference
parallel.py:300-369) against tests/genotype_match_ref.py, a plain restatement of the rule - on the host tier and on the GPU, in the wave
and the thread form, with the grid of the match capped at 1 / 2 / 7 workgroups and uncapped.  `best` and `dist` are compared with ==.
The tables (tests/genotype_match_cases.py) state per scenario what they expect and assert from the restatement that they sit on the
edge they are named after; the restatement itself is held against the matches the unmodified reference recorded
(tests/golden/genotype_targets.json.gz) and, where the reference is available, against its own `GenotypeTask.execute`."""
import numpy as np
import pytest

import genotype_match_cases as GC
import genotype_match_ref as R
import golden_util as gu
from sniffles_amd import lib

TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]
FORMS = {"wave": 0, "thread": 1}
GRIDS = (1, 2, 7, 0)
_cache = {}


def use_tier(tier):
    if tier == "host":
        import emu.emu as EM
        EM.lib()                                         # the host tier becomes the library of this test
    else:
        assert lib.device_count() >= 1


def built(name, make):
    """A case and the restatement's answer for it, once per session."""
    if name not in _cache:
        k = make()
        best, dist = R.match(k.c, k.t, k.cfg)
        assert best == k.expect, (k.name, [i for i, (a, b) in enumerate(zip(best, k.expect)) if a != b][:8])
        _cache[name] = (k, np.asarray(best, np.int32), np.asarray(dist, np.int32))
    return _cache[name]


def run(k, want_best, want_dist, forms=FORMS, grids=GRIDS):
    for form in forms:
        for max_grid in grids:
            best, dist = lib.genotype_match_batch(k.cfg, k.c, k.t, max_grid=max_grid, form=FORMS[form])
            assert np.array_equal(best, want_best), (k.name, form, max_grid, np.flatnonzero(best != want_best)[:8])
            assert np.array_equal(dist, want_dist), (k.name, form, max_grid, np.flatnonzero(dist != want_dist)[:8])
            st = lib.genotype_match_last_stats()
            per = 256 if FORMS[form] else 4
            full = min(65536, -(-len(want_best) // per))
            assert (st["targets"], st["candidates"]) == (len(want_best), len(k.c["pos"]))
            assert st["workgroups"] == (min(full, max_grid) if max_grid else full)


@pytest.mark.parametrize("name", ["bin_rule", "ties", "other_gates", "bnd", "types", "populations"])
@pytest.mark.parametrize("tier", TIERS)
def test_directed_tables(tier, name):
    use_tier(tier)
    k, best, dist = built(name, getattr(GC, name))
    assert (best >= 0).any() and ((best < 0).any() or name == "ties")      # (every tie has a winner)
    run(k, best, dist)


@pytest.mark.parametrize("cm", [1, 3, 7, 33, 250])
@pytest.mark.parametrize("tier", TIERS)
def test_root_gate_at_floor_and_floor_plus_one(tier, cm):
    """dist = floor(combine_match * sqrt(minlen)) matches and floor + 1 does not, for minlen 1 .. 4096 (GPU: every value; host tier:
    the perfect squares, their neighbours and every 16th value)."""
    use_tier(tier)
    minlens = GC.host_minlens() if tier == "host" else range(1, 4097)
    k, best, dist = built(f"root_gate_{cm}_{tier}", lambda: GC.root_gate(cm, minlens))
    assert int((best >= 0).sum()) == int((best < 0).sum()) == 3 * len(minlens)
    run(k, best, dist)


@pytest.mark.parametrize("tier", TIERS)
def test_empty_sides(tier):
    use_tier(tier)
    a, b = GC.empty_sides()
    for form in FORMS.values():
        best, dist = lib.genotype_match_batch(a.cfg, a.c, a.t, form=form)
        assert best.tolist() == [-1] * 4 and dist.tolist() == [0] * 4
        best, dist = lib.genotype_match_batch(b.cfg, b.c, b.t, form=form)
        assert len(best) == len(dist) == 0


@pytest.mark.parametrize("tier", TIERS)
def test_target_counts_around_the_capped_grid(tier):
    """n_targets on either side of max_grid x waves per workgroup (the wave form's targets per round) and of its next multiple; the
    thread form around one and two workgroups' worth."""
    use_tier(tier)
    k, best, dist = built("populations", GC.populations)
    tiled = GC.Case("tiled", **k.options)
    tiled.c = k.c
    reps = -(-520 // len(best))
    tiled.t = {key: v * reps for key, v in k.t.items()}
    want_b, want_d = np.tile(best, reps), np.tile(dist, reps)
    for max_grid in (1, 2, 7):
        for n in sorted({max_grid * 4 * m + e for m in (1, 2) for e in (-1, 0, 1)}):
            run(tiled.head(n), want_b[:n], want_d[:n], forms=("wave",), grids=(max_grid,))
    for n in (255, 256, 257, 511, 512, 513):
        run(tiled.head(n), want_b[:n], want_d[:n], forms=("thread",), grids=(1,))


# ---------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("name", ["bnd_stale_end", "chr20_30x_ont", "chr21_30x_mosaic", "fuzz_4_2", "long_ins"])
def test_restatement_against_the_recorded_reference(name):
    """tests/genotype_match_ref.py against `match` / `dist` of the unmodified reference's GenotypeTask.execute (golden)."""
    import cases
    doc = gu.load("genotype_targets")[name]
    cand = gu.load(name)["expected"]["candidates"]
    cfg = gu.make_config(cases.ALL[name][1], cases.ALL[name][0]())
    c, t = R.tables_from_records(cand, doc["specs"])
    best, dist = R.match(c, t, cfg)
    got = [(None, None) if b < 0 else (cand[b]["id"], float(d)) for b, d in zip(best, dist)]
    assert got == [(w["match"], w["dist"]) for w in doc["expected"]["targets"]]
    if name != "long_ins":
        assert any(b >= 0 for b in best) and any(b < 0 for b in best)


@pytest.mark.skipif(not __import__("make_ref").ref_root(), reason="needs the reference (its checkout, or the staged build oracle/_ref that make_ref.py compiles)")
def test_restatement_against_the_reference_itself():
    """The restatement against the unmodified reference's own GenotypeTask.execute on random tasks and target sets (host tier only)."""
    import genotype_util as gutil
    import ref_harness as rh
    from sniffles_amd import synth
    n_targets = n_matched = 0
    for it in range(6):
        ti = synth.gen_fuzz(310000 + it, task_id=it % 4)
        ref_run = rh.run_reference(ti, ())
        if "error" in ref_run:
            continue
        specs = gutil.target_specs(ref_run["candidates"], ti.contig_len, 900 + it)
        exp = rh.run_reference_genotype(ti, specs, ())
        if not specs or "error" in exp:
            continue
        cfg = gu.make_config({}, ti)
        c, t = R.tables_from_records(ref_run["candidates"], specs)
        best, dist = R.match(c, t, cfg)
        got = [(None, None) if b < 0 else (ref_run["candidates"][b]["id"], float(d)) for b, d in zip(best, dist)]
        assert got == [(w["match"], w["dist"]) for w in exp["targets"]], it
        n_targets += len(best)
        n_matched += sum(1 for b in best if b >= 0)
    assert n_targets > 50 and n_matched > 5
