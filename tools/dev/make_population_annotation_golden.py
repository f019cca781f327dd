#!/usr/bin/env python3
"""Build-container script: tests/golden/popannot_4samples.json.gz - a population SNF and three annotated merges, everything
written by the UNMODIFIED reference (oracle/ref_harness.py loads it; edlib replaced by the exact DP of the C oracle, as everywhere).

  population A   cases.POPULATIONS["population_4samples_12x"] (seeds 30..33, chr8 / chr9, coverage 12, site_seed 77): each BAM ->
                 .snf, merged, the merged calls stored through the reference's own `PopulationSNF` the way
                 `CombineResultTmpFilePopulationSNF.finalize` does it (result.py:266-277: per task `store` in emission order,
                 `write_and_index`; `add_result`; then `write_results`, sniffles:565-568)
  population B   seeds 40..42 of the same generator, merged with `--combine-population` against that file for three option sets

The document holds the input hashes of A and B, the population file (base64), the three VCF texts and per text the counts
(records, matched, unmatched), which tests/test_population_annotation.py asserts as well - a fixture that annotates nothing cannot
pass.  Two things the reference needs to get through this in one process: `sniffles.snfp.align` patched like `sniffles.sv.align`
(snfp.py imports edlib on its own), and `config.combine_population` set back to the path before every task -
`CombineTask.execute` replaces the path by the opened object (parallel.py:454-455) and the next task fails on it.

    python tools/dev/make_population_annotation_golden.py
"""
import base64
import gzip
import io
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OPTION_SETS = {"default": (), "match3_pctseq097": ("--combine-match", "3", "--combine-pctseq", "0.97"), "pctseq0": ("--combine-pctseq", "0")}
POPULATION_B_SEEDS = (40, 41, 42)


def population_b():
    import cases
    return [cases._sample(s, ref_names=("chr8", "chr9"), ref_lens=(1_000_000, 1_000_050), cov=12.0, site_seed=77, site_spacing=12000)
            for s in POPULATION_B_SEEDS]


def counts(vcf_text: str) -> list:
    """[records, matched, unmatched]: a matched record carries a float POPULATION_AF, an unmatched one the int 0."""
    import vcf_util as vu
    body = vu.split_text(vcf_text)[1]
    matched = sum(1 for ln in body if ";POPULATION_AF=" in ln and ";POPULATION_AF=0;" not in ln)
    unmatched = sum(1 for ln in body if ";POPULATION_AF=0;POPULATION_SIZE=0;" in ln)
    assert matched + unmatched == len(body)
    return [len(body), matched, unmatched]


def reference_merge(rh, paths, extra_args, fixed, population=None, population_out=None):
    """The reference's `combine` flow in this process (as ref_harness.run_reference_population runs it) over the sample files
    `paths`; `population`: --combine-population; `population_out`: the merged calls also go into a population SNF there.
    Returns (vcf text, variants stored, merged calls)."""
    import oracle as oc
    ref = rh.load_reference()
    from sniffles import snf as ref_snf, snfp as ref_snfp, vcf as ref_vcf
    dp = lambda a, b, **kw: {"editDistance": oc.edit_distance(a.encode("latin-1"), b.encode("latin-1"))}  # noqa: E731
    ref.sv.align = dp
    ref_snfp.align = dp
    args = list(extra_args) + (["--combine-population", population] if population else []) + \
        (["--dev-population-snf", population_out] if population_out else [])
    cfg = ref.config.SnifflesConfig("--input", *paths, "--vcf", "out.vcf", *args)
    cfg.mode = "combine"
    for k, v in fixed.items():
        setattr(cfg, k, v)
    cfg.snf_input_info = []
    contig_lengths = None
    for internal_id, path in enumerate(paths):
        f = ref_snf.SNFile(cfg, open(path, "rb"), filename=path)
        f.read_header()
        contig_lengths = f.header["config"]["contig_lengths"]
        sid = f.header["config"]["sample_id"] or os.path.splitext(os.path.basename(path))[0]
        cfg.snf_input_info.append({"internal_id": internal_id, "sample_id": sid, "filename": path})
        f.close()
    cfg.sample_ids_vcf = [(i["internal_id"], i["sample_id"]) for i in cfg.snf_input_info]
    cfg.combine_close_handles = False
    buf = io.StringIO()
    w = ref_vcf.VCF(cfg, buf)
    w.write_header(contig_lengths)

    class Collector:
        def __init__(self, task, svcalls, count):
            self.calls = []

        def store_calls(self, svcalls):
            self.calls.extend(svcalls)

        def finalize(self):
            pass
    psnf_out = ref_snfp.PopulationSNF(cfg, open(population_out, "wb")) if population_out else None
    stored = merged = 0
    for task_id, (contig, length) in enumerate(contig_lengths):
        cfg.combine_population = population          # (execute replaces the path by the opened file)
        task = ref.parallel.CombineTask(id=task_id, sv_id=0, contig=contig, start=0, end=length - 1, assigned_process_id=None,
                                        config=cfg, result_class=Collector, regions=None)
        res = task.execute()
        merged += len(res.calls)
        if psnf_out is not None:
            part_name = f"{population_out}.tmp_{task_id}.snf"
            with open(part_name, "wb") as handle:
                part = ref_snfp.PopulationSNF(cfg, handle)
                c = sum(1 for call in res.calls if part.store(call))
                part.write_and_index()
            stored += c
            psnf_out.add_result(types.SimpleNamespace(has_snf=True, task_id=task_id, contig=contig, snf_filename=part_name,
                                                      snf_index=part.get_index(), snf_total_length=part.get_total_length(),
                                                      snf_candidate_count=c))
        for c in sorted(res.calls, key=lambda c: c.pos):
            w.write_call(c)
    if psnf_out is not None:
        psnf_out.write_results(cfg, [c for c, _ in contig_lengths])
        psnf_out.close()
    return buf.getvalue(), stored, merged


def sample_files(rh, recs_list, workdir, fixed) -> list:
    paths = []
    for s, recs in enumerate(recs_list):
        path = os.path.join(workdir, f"sample{s}.snf")
        rh.run_reference_call_sample(recs, (), path, fixed)
        paths.append(path)
    return paths


def main():
    import cases
    import ref_harness as rh
    import vcf_util as vu
    from extract_util import records_sha
    work = tempfile.mkdtemp(prefix="popannot_")
    recs_a = cases.POPULATIONS["population_4samples_12x"][0]()
    recs_b = population_b()
    dir_a, dir_b = os.path.join(work, "a"), os.path.join(work, "b")
    os.makedirs(dir_a); os.makedirs(dir_b)
    pop_path = os.path.join(work, "population.snf")
    _, stored, merged = reference_merge(rh, sample_files(rh, recs_a, dir_a, vu.FIXED), (), vu.FIXED, population_out=pop_path)
    with open(pop_path, "rb") as f:
        pop_bytes = f.read()
    paths_b = sample_files(rh, recs_b, dir_b, vu.FIXED)
    vcfs = {name: reference_merge(rh, paths_b, args, vu.FIXED, population=pop_path)[0] for name, args in OPTION_SETS.items()}
    doc = dict(input_sha_a=[records_sha(r) for r in recs_a], input_sha_b=[records_sha(r) for r in recs_b],
               population_snf=base64.b64encode(pop_bytes).decode(), population_stored=[stored, merged],
               options={k: list(v) for k, v in OPTION_SETS.items()}, vcf=vcfs, counts={k: counts(v) for k, v in vcfs.items()})
    out = os.path.join(ROOT, "tests", "golden", "popannot_4samples.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, sort_keys=True, separators=(",", ":")).encode())
    print(f"population file {len(pop_bytes)} bytes, {stored} of {merged} merged calls stored")
    for k, v in doc["counts"].items():
        print(f"{k:20s} records {v[0]}, matched {v[1]}, unmatched {v[2]}")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
