"""`--combine-population` and `--dev-population-snf` end to end against data written by the UNMODIFIED reference
(tests/golden/popannot_4samples.json.gz, made by tools/dev/make_population_annotation_golden.py): population A (cases.POPULATIONS
["population_4samples_12x"]) merged and stored by the reference's own `PopulationSNF`, population B (seeds 40..42 of the same generator)
merged against that file with three option sets - every merged call carries POPULATION_AF / POPULATION_SIZE of its best-matching
variant.  Here: B's samples BAM -> .snf by this package, `pipeline.combine` against the committed file - the VCF text character by
character, on all three paths of the merge; A merged with `dev_population_snf` - the file read back equals the reference's, variant by
variant, and annotates B to the same three texts; a file whose index lists two parts for one block.  Host tier, and the MI355X."""
import base64
import io
import os
import pickle
import tempfile

import pytest

import cases
import golden_util as gu
from extract_util import records_sha
from sniffles_amd import lib, pipeline, snfp, sv
from test_pipeline import config_for

TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]
OPTION_SETS = {"default": (), "match3_pctseq097": ("--combine-match", "3", "--combine-pctseq", "0.97"), "pctseq0": ("--combine-pctseq", "0")}
COUNTS = {"default": [151, 149, 2], "match3_pctseq097": [168, 141, 27], "pctseq0": [151, 149, 2]}      # records, matched, unmatched
_samples = {}      # (tier, population) -> paths of the samples' .snf files (this package's, written once per session)


def use_tier(tier):
    if tier == "host":
        import emu.emu as EM
        EM.lib()                                         # the host tier becomes the library of this test
    else:
        assert lib.device_count() >= 1


def population_b():
    return [cases._sample(s, ref_names=("chr8", "chr9"), ref_lens=(1_000_000, 1_000_050), cov=12.0, site_seed=77, site_spacing=12000)
            for s in (40, 41, 42)]


def doc():
    return gu.load("popannot_4samples")


def sample_files(tier, which) -> list:
    """The per-sample .snf files of population A or B (BAM -> .snf by this package on the tier's library)."""
    if (tier, which) not in _samples:
        recs = cases.POPULATIONS["population_4samples_12x"][0]() if which == "a" else population_b()
        assert [records_sha(r) for r in recs] == doc()["input_sha_" + which]
        d = tempfile.mkdtemp(prefix=f"popannot_{tier}_{which}_")
        paths = []
        for k, r in enumerate(recs):
            paths.append(os.path.join(d, f"sample{k}.snf"))
            pipeline.call_sample(r, config_for(()), snf_path=paths[-1], tandem_repeats=getattr(r, "tandem_repeats", None))
        _samples[(tier, which)] = paths
    return _samples[(tier, which)]


def committed_population(tmp_path) -> str:
    path = str(tmp_path / "population.snf")
    with open(path, "wb") as f:
        f.write(base64.b64decode(doc()["population_snf"]))
    return path


def counts(text: str) -> list:
    body = [ln for ln in text.splitlines() if not ln.startswith("#")]
    matched = sum(1 for ln in body if ";POPULATION_AF=" in ln and ";POPULATION_AF=0;" not in ln)
    unmatched = sum(1 for ln in body if ";POPULATION_AF=0;POPULATION_SIZE=0;" in ln)
    return [len(body), matched, unmatched]


def merged_text(paths, args, population, objects=True, **extra):
    cfg = config_for(tuple(args))
    cfg.combine_population = population
    for k, v in extra.items():
        setattr(cfg, k, v)
    buf = io.StringIO()
    calls = pipeline.combine(paths, cfg, vcf_handle=buf, objects=objects)
    assert cfg.combine_population is population          # the caller's config keeps what it was given
    assert (calls == []) == (not objects)
    return buf.getvalue(), calls


def check_three_texts(paths, population):
    d = doc()
    for name, args in OPTION_SETS.items():
        want = d["vcf"][name]
        assert d["counts"][name] == COUNTS[name] == counts(want)
        text, calls = merged_text(paths, args, population)
        assert text == want, name
        # the objects carry the reference's types: a float and an int, or the two ints (0, 0)
        unmatched = [c for c in calls if c.info["POPULATION_SIZE"] == 0]
        assert all(isinstance(c.info["POPULATION_AF"], int) and c.info["POPULATION_AF"] == 0 for c in unmatched) and len(unmatched) >= COUNTS[name][2]
        assert all(isinstance(c.info["POPULATION_AF"], float) and isinstance(c.info["POPULATION_SIZE"], int) for c in calls if c not in unmatched)
        assert merged_text(paths, args, population, objects=False)[0] == want, name      # straight from the group table
    return d


@pytest.mark.parametrize("tier", TIERS)
def test_merge_against_the_reference_written_population(tier, tmp_path, monkeypatch):
    use_tier(tier)
    paths = sample_files(tier, "b")
    population = committed_population(tmp_path)
    d = check_three_texts(paths, population)
    # an opened file instead of the path (what the reference's CombineTask.execute puts into its config)
    opened = snfp.PopulationSNF.open(population, config_for(()))
    assert merged_text(paths, (), opened)[0] == d["vcf"]["default"]
    # the object-by-object twin of the merge
    monkeypatch.setenv("SNF_COMBINE_OBJECTS", "1")
    assert merged_text(paths, (), population)[0] == d["vcf"]["default"]
    monkeypatch.delenv("SNF_COMBINE_OBJECTS")
    # without the option: no header lines, no fields (and the same records otherwise)
    plain = merged_text(paths, (), None)[0]
    assert "POPULATION" not in plain
    strip = lambda t: [ln.split(";POPULATION_AF=")[0] + ";STDEV_LEN=" + ln.split(";STDEV_LEN=", 1)[1] for ln in t.splitlines() if not ln.startswith("#")]  # noqa: E731
    assert strip(d["vcf"]["default"]) == [ln for ln in plain.splitlines() if not ln.startswith("#")]


def file_content(f) -> dict:
    """{contig: {block key: [ {svtype: [attribute dicts]} per part ]}} of an opened population file."""
    out = {}
    for contig, blocks in f.index.items():
        out[contig] = {}
        for key in blocks:
            out[contig][key] = [{t: [dict(vars(v)) for v in part[t]] for t in part if t != "_COVERAGE"} for part in f.read_blocks(contig, key)]
    return out


@pytest.mark.parametrize("tier", TIERS)
def test_population_file_written_here_equals_the_reference_written_one(tier, tmp_path):
    use_tier(tier)
    ours = str(tmp_path / "ours.snf")
    cfg = config_for(())
    cfg.dev_population_snf = ours
    calls = pipeline.combine(sample_files(tier, "a"), cfg, vcf_handle=io.StringIO())
    d = doc()
    assert d["population_stored"] == [156, 158] and len(calls) == 158
    mine, theirs = snfp.PopulationSNF.open(ours, config_for(())), snfp.PopulationSNF.open(committed_population(tmp_path), config_for(()))
    assert mine.population == theirs.population == snfp.PopulationInfo(version=1, name="Population", description="A sample population", size=4)
    assert mine.header["snf_candidate_count"] == theirs.header["snf_candidate_count"] == 156
    assert mine.header["config"]["contig_coverages"] == theirs.header["config"]["contig_coverages"] == {}
    assert {c: sorted(b) for c, b in mine.index.items()} == {c: sorted(b) for c, b in theirs.index.items()} and list(mine.index) == list(theirs.index)
    got, want = file_content(mine), file_content(theirs)
    assert got == want
    variants = [v for c in want.values() for parts in c.values() for part in parts for vs in part.values() for v in vs]
    assert len(variants) == 156 and all("rnames" in v and v["rnames"] is None for v in variants)
    assert set(want["chr8"][next(iter(want["chr8"]))][0]) == set(sv.TYPES)
    # the same annotation from OUR file; without objects the population file is written all the same
    check_three_texts(sample_files(tier, "b"), ours)
    again = str(tmp_path / "again.snf")
    cfg = config_for(())
    cfg.dev_population_snf = again
    assert pipeline.combine(sample_files(tier, "a"), cfg, vcf_handle=io.StringIO(), objects=False) == []
    assert file_content(snfp.PopulationSNF.open(again, config_for(()))) == want


needs_ref = pytest.mark.skipif(not __import__("make_ref").ref_root(), reason="needs the reference (its checkout, or the staged build oracle/_ref that make_ref.py compiles)")


@needs_ref
def test_reference_reads_the_population_file_written_here(tmp_path, oracle_mod):
    """The unmodified reference's `PopulationSNF.open` + `get_population_AF` on OUR file agrees with ours on every merged call of B; its
    unpickler finds real `sniffles.snfp.PopulationVariant` records in it."""
    import ref_harness as rh
    use_tier("host")
    ours = str(tmp_path / "ours.snf")
    cfg = config_for(())
    cfg.dev_population_snf = ours
    pipeline.combine(sample_files("host", "a"), cfg, vcf_handle=io.StringIO())
    calls = pipeline.combine(sample_files("host", "b"), config_for(()))
    assert len(calls) > 150
    mine = snfp.PopulationSNF.open(ours, config_for(()))
    af, size = mine.get_population_AF_batch(calls)
    rh.load_reference()
    from sniffles import snfp as ref_snfp
    rh.make_config(())                                   # (SnifflesConfig.__init__ makes it SnifflesConfig.GLOBAL, config.py:619)
    keep = ref_snfp.align
    ref_snfp.align = lambda a, b, **kw: {"editDistance": oracle_mod.edit_distance(a.encode("latin-1"), b.encode("latin-1"))}
    try:
        theirs = ref_snfp.PopulationSNF.open(ours)
        assert theirs.header["population"] == ref_snfp.PopulationInfo(version=1, name="Population", description="A sample population", size=4)
        want = [theirs.get_population_AF(c) for c in calls]
        first = next(iter(theirs._blocks["chr8"].values()))
        assert any(type(v) is ref_snfp.PopulationVariant for vs in first.values() if isinstance(vs, list) for v in vs)
    finally:
        ref_snfp.align = keep
    got = [None if a != a else (a, s) for a, s in zip(af.tolist(), size.tolist())]
    assert got == want and sum(w is None for w in want) >= 2 and sum(w is not None for w in want) > 140
    # and a block of ours unpickles with the standard library alone under the reference's modules
    with open(ours, "rb") as f:
        header = f.readline()
        import gzip
        import json
        start, length = json.loads(header)["index"]["chr8"][next(iter(json.loads(header)["index"]["chr8"]))][0]
        f.seek(len(header) + start)
        block = pickle.loads(gzip.decompress(f.read(length)))
    assert all(type(v).__module__ == "sniffles.snfp" for vs in block.values() if isinstance(vs, list) for v in vs)
