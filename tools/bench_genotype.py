"""Force calling (`pipeline.genotype_vcf`) through `SVCall` objects against the record path (`objects=False`), alternating in one
session on one sample: wall time per contig split into reading the targets / extraction / pass + match + coverage / text, the
spread over the rounds, the HIP-event time of the match chain (keys, sort, match) inside the record path and of the stand-alone
entry on the same tables.  The sample is `synth_bam.gen_sample` at its default size, the targets its own `call_sample` VCF
concatenated with a copy shifted by 180 bp, so that near misses exist.

    python tools/bench_genotype.py [--rounds 5] [--log profiles/genotype_records_ab.log] [--json profiles/genotype_records_bench.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--scale", type=float, default=1.0, help="contig lengths of the sample relative to gen_sample's default")
    ap.add_argument("--host-tier", action="store_true", help="plumbing check on the test suite's host build of the kernels (never a measurement)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from sniffles_amd import bam, lib, pipeline, synth_bam, vcf
    from sniffles_amd.config import SnifflesConfig
    if a.host_tier:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import emu.emu as E
        E.lib()
    ref_lens = tuple(max(1_000_001, int(n * a.scale)) if n >= 1_000_000 else n for n in (1_400_000, 16_000, 1_100_000))
    names, lens, recs = synth_bam.gen_sample(a.seed, ref_lens=ref_lens)[:3]
    records = bam.parse_bam(bam.bam_stream(names, lens, recs))

    start_date = SnifflesConfig().start_date

    def config():
        cfg = SnifflesConfig()
        cfg.start_date = start_date          # (the header's date line: the same in every run, so that the texts can be compared)
        return cfg
    buf = io.StringIO()
    pipeline.call_sample(records, config(), vcf_handle=buf, objects=False)
    lines = buf.getvalue().split("\n")
    body = [ln for ln in lines if ln and not ln.startswith("#")]
    moved = []
    for ln in body:
        c = ln.split("\t")
        c[1] = str(int(c[1]) + 180)
        moved.append("\t".join(c))
    vcf_in = "\n".join([ln for ln in lines if ln.startswith("#")] + body + moved) + "\n"
    n_contigs = sum(1 for c, n in zip(names, lens) if pipeline.should_process_contig(c, int(n), config()))
    out_lines = []

    def say(text):
        print(text, flush=True)
        out_lines.append(text)
    say(f"# sample: {len(recs)} records on {list(zip(names, [int(x) for x in lens]))}, {n_contigs} contigs processed; targets: {len(body)} calls + {len(moved)} shifted copies")
    runs = {True: [], False: []}
    texts = {}
    for rnd in range(a.rounds + 1):          # round 0 warms both paths up (library load, arenas, first-use allocations)
        for objects in ((True, False) if rnd % 2 == 0 else (False, True)):
            tm = {}
            o = io.StringIO()
            t0 = time.perf_counter()
            n = pipeline.genotype_vcf(records, config(), io.StringIO(vcf_in), o, objects=objects, timing=tm)
            tm["wall"] = time.perf_counter() - t0
            texts[objects] = o.getvalue()
            if rnd:
                runs[objects].append(tm)
            say(f"round {rnd} objects={objects}: {n} records, per contig ms: " +
                " ".join(f"{k}={tm[k] * 1e3 / n_contigs:.2f}" for k in ("wall", "read", "extract", "pass_match", "text")) +
                f" match_kernel_ms={tm['match_kernel_ms'] / n_contigs:.4f}")
    assert texts[True] == texts[False], "the two paths wrote different text"

    def stat(objects, key):
        v = [r[key] * 1e3 / n_contigs for r in runs[objects]]
        return dict(median=statistics.median(v), min=min(v), max=max(v))
    res = {"rounds": a.rounds, "contigs": n_contigs, "bam_records": len(recs), "targets": len(body) + len(moved), "same_text": True,
           "per_contig_ms": {("objects" if o else "records"): {k: stat(o, k) for k in ("wall", "read", "extract", "pass_match", "text")} for o in (True, False)},
           "match_chain_kernel_ms_per_contig": statistics.median(r["match_kernel_ms"] / n_contigs for r in runs[False])}
    w_o, w_r = res["per_contig_ms"]["objects"]["wall"], res["per_contig_ms"]["records"]["wall"]
    res["records_over_objects_wall"] = w_r["median"] / w_o["median"]
    res["spread_objects"] = (w_o["max"] - w_o["min"]) / w_o["median"]
    res["spread_records"] = (w_r["max"] - w_r["min"]) / w_r["median"]
    # the stand-alone entry on one contig's tables: candidates = targets of that contig (the sample's own calls), both forms
    t = vcf.VCF(config(), io.StringIO(vcf_in)).read_target_table()
    first = next(iter(t.values()))
    cols = dict(svtype=first["svtype"], pos=first["pos"], svlen=first["svlen"], mate_contig=first["mate_contig"])
    alone = {}
    for form, name in ((0, "wave"), (1, "thread")):
        ms = []
        for _ in range(6):
            lib.genotype_match_batch(config(), cols, cols, form=form)
            ms.append(lib.genotype_match_last_stats()["kernel_ms"])
        alone[name] = dict(targets=len(cols["pos"]), candidates=len(cols["pos"]), kernel_ms_median=statistics.median(ms[1:]), kernel_ms_min=min(ms[1:]))
    res["stand_alone_match"] = alone
    say(json.dumps(res))
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(out_lines) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
