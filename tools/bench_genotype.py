"""Force calling (`pipeline.genotype_vcf`) through `SVCall` objects against the record path (`objects=False`), alternating in one
session on one sample: wall time per contig split into reading the targets / extraction / pass + match + coverage / text, the
spread over the rounds, the HIP-event time of the match chain (keys, sort, match) inside the record path and of the stand-alone
entry on the same tables.  The sample is `synth_bam.gen_sample` at its default size, the targets its own `call_sample` VCF
concatenated with a copy shifted by 180 bp, so that near misses exist.

    python tools/bench_genotype.py [--rounds 5] [--log profiles/genotype_records_ab.log] [--json profiles/genotype_records_bench.json]

`--targets N`: the two text stages on their own, on a SYNTHETIC, seeded, cohort-shaped target VCF of N records (half of them INS with
inline ALT sequences, 3 % BND, Sniffles-style INFO, ten sample columns; no sample behind it): `read_target_table` +
`rewrite_genotype_records` (the parent path) alternating with `read_target_table_device` + `rewrite_genotype_device` over the same bytes,
with made-up genotype rows, the texts compared; medians and max - min of `read` and `text`, the kernels' share, and the text's bytes over
the time of vt_lines + vt_parse against the HBM copy rate (MI355X: 6.29 TB/s measured, 8 TB/s spec).

    python tools/bench_genotype.py --targets 200000 [--rounds 5] [--log profiles/target_text_ab.log] [--json profiles/target_text_bench.json]
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


HBM_COPY_BYTES_PER_S = 6.29e12      # MI355X, float4 copy (8.0e12 spec)


def synthetic_targets(n: int, seed: int) -> bytes:
    """A cohort-shaped target VCF of n records: SYNTHETIC (seeded, no sample behind it).  24 contigs in order, positions rising."""
    import numpy as np
    rng = np.random.default_rng(seed)
    contigs = ["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY"]
    samples = ["S%02d" % k for k in range(10)]
    out = ["##fileformat=VCFv4.2", "##source=synthetic cohort-shaped targets (tools/bench_genotype.py --targets, seed %d)" % seed]
    out += ["##contig=<ID=%s,length=%d>" % (c, 250_000_000) for c in contigs]
    out += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]
    per = [n // len(contigs) + (1 if k < n % len(contigs) else 0) for k in range(len(contigs))]
    kind = rng.random(n)
    length = np.minimum(50 + rng.geometric(1 / 400.0, n), 20_000)
    bases = np.frombuffer(b"ACGT", np.uint8)
    gts = ["0/0:60:30:0:NULL", "0/1:45:14:12:Sniffles2.INS.1S0", "1/1:60:0:25:Sniffles2.DEL.2S0", "./.:0:0:0:NULL"]
    i = 0
    for c, m in zip(contigs, per):
        pos = np.sort(rng.integers(10_000, 240_000_000, m))
        for p in pos.tolist():
            L = int(length[i])
            sup = int(rng.integers(2, 60))
            tail = "SUPPORT=%d;COVERAGE=%d,%d,%d,%d,%d;STRAND=+-;AC=%d;SUPP_VEC=%s;STDEV_LEN=%.3f;STDEV_POS=%.3f;VAF=%.3f" % (
                sup, *rng.integers(5, 60, 5).tolist(), int(rng.integers(1, 20)), "".join(rng.choice(["0", "1"], 10).tolist()), rng.random() * 9, rng.random() * 9, rng.random())
            k = kind[i]
            if k < 0.5:
                alt = "N" + rng.choice(bases, L).tobytes().decode()
                row = [c, str(p), "Sniffles2.INS.%XM%d" % (i, 0), "N", alt, "60", "PASS", "PRECISE;SVTYPE=INS;SVLEN=%d;END=%d;%s" % (L, p, tail)]
            elif k < 0.53:
                mate = contigs[int(rng.integers(0, len(contigs)))]
                form = ("N[%s:%d[", "N]%s:%d]", "]%s:%d]N", "[%s:%d[N")[int(rng.integers(0, 4))] % (mate, int(rng.integers(10_000, 240_000_000)))
                row = [c, str(p), "Sniffles2.BND.%XM%d" % (i, 0), "N", form, "60", "PASS", "IMPRECISE;SVTYPE=BND;CHR2=%s;%s" % (mate, tail)]
            else:
                t = ("DEL", "DEL", "DEL", "DUP", "INV")[int(rng.integers(0, 5))]
                row = [c, str(p), "Sniffles2.%s.%XM%d" % (t, i, 0), "N", "<%s>" % t, "60", "PASS",
                       "PRECISE;SVTYPE=%s;SVLEN=%d;END=%d;%s" % (t, -L if t == "DEL" else L, p + L, tail)]
            out.append("\t".join(row + ["GT:GQ:DR:DV:ID"] + [gts[int(g)] for g in rng.integers(0, len(gts), len(samples)).tolist()]))
            i += 1
    return ("\n".join(out) + "\n").encode()


def targets_bench(a):
    """`--targets N`: parent text stages against the device's, alternating, over one synthetic text."""
    import types

    import numpy as np
    from sniffles_amd import abi, parallel, vcf
    from sniffles_amd.config import SnifflesConfig
    if a.host_tier:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import emu.emu as E
        E.lib()
    out_lines = []

    def say(text):
        print(text, flush=True)
        out_lines.append(text)
    t0 = time.perf_counter()
    data = synthetic_targets(a.targets, a.seed)
    say(f"# SYNTHETIC target VCF (seed {a.seed}): {a.targets} records, {len(data)} bytes, generated in {time.perf_counter() - t0:.1f} s"
        + (" - HOST TIER: a plumbing check, not a measurement" if a.host_tier else ""))
    cfg = SnifflesConfig()
    stub = types.SimpleNamespace(config=cfg, _ti=types.SimpleNamespace(ps_name=lambda code: str(code)))
    to_tuples = lambda g: parallel.GenotypeTask.genotype_tuples(stub, {"gt": g})      # noqa: E731
    kinds = np.asarray([(0, 1, 30, 5, 6, -1, -1, abi.GTSRC_MATCH), (1, 1, 60, 0, 9, -1, -1, abi.GTSRC_MATCH), (0, 0, 0, 17, 0, -1, -1, abi.GTSRC_DEPTH),
                        (0, 0, 0, 0, 0, -1, -1, abi.GTSRC_NONE)] + [(0, 1, 20 + k, 9, k, -1, -1, abi.GTSRC_MATCH) for k in range(40)], np.int32)
    rng = np.random.default_rng(a.seed + 1)

    def parent():
        tm = {}
        t0 = time.perf_counter()
        reader = vcf.VCF(cfg, io.BytesIO(data))
        tab = reader.read_target_table()
        tm["read"] = time.perf_counter() - t0
        gts = {c: kinds[rng_pick[c]] for c in tab}
        tuples = {c: to_tuples(gts[c]) for c in tab}      # (outside the text stage: the genotype tuples come from the task in the driver)
        o = io.TextIOWrapper(io.BytesIO(), encoding="utf-8", newline="\n")      # (what open(path, "w") is, without the disk)
        t0 = time.perf_counter()
        w = vcf.VCF(cfg, o)
        for c, t in tab.items():
            w.rewrite_genotype_records(t["lines"], tuples[c])
        o.flush()
        tm["text"] = time.perf_counter() - t0
        return tm, o.buffer.getvalue(), reader.header_str

    def device():
        tm = {}
        t0 = time.perf_counter()
        reader = vcf.VCF(cfg, None)
        tab = reader.read_target_table_device(data)
        tm["read"] = time.perf_counter() - t0
        tm["lines_ms"], tm["parse_ms"], tm["n_host_lines"] = reader.target_timing["lines_ms"], reader.target_timing["parse_ms"], reader.n_host_lines
        o = io.TextIOWrapper(io.BytesIO(), encoding="utf-8", newline="\n")      # (what open(path, "w") is, without the disk)
        t0 = time.perf_counter()
        w = vcf.VCF(cfg, o)
        ms = 0.0
        for c, t in tab.items():
            w.rewrite_genotype_device(t["lines"], None, kinds[rng_pick[c]], tuples=to_tuples)
            ms += w.rewrite_kernel_ms
        o.flush()
        tm["text"] = time.perf_counter() - t0
        tm["rewrite_ms"] = ms
        for t in tab.values():
            t["lines"].text.close()
        return tm, o.buffer.getvalue(), reader.header_str

    first = vcf.VCF(cfg, io.BytesIO(data)).read_target_table()
    rng_pick = {c: rng.integers(0, len(kinds), len(t["pos"])) for c, t in first.items()}
    del first
    runs = {"parent": [], "device": []}
    texts = {}
    for rnd in range(a.rounds + 1):          # round 0 warms both paths up
        for name, fn in ((("parent", parent), ("device", device)) if rnd % 2 == 0 else (("device", device), ("parent", parent))):
            tm, text, header = fn()
            texts[name] = (text, header)
            if rnd:
                runs[name].append(tm)
            say(f"round {rnd} {name}: " + " ".join(f"{k}={v * 1e3:.1f}ms" if k in ("read", "text") else f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in tm.items()))
    assert texts["parent"] == texts["device"], "the two paths gave different text"

    def stat(name, key, scale=1e3):
        v = [r[key] * scale for r in runs[name]]
        return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))
    res = {"synthetic": True, "seed": a.seed, "records": a.targets, "bytes": len(data), "rounds": a.rounds, "same_text": True, "host_tier": bool(a.host_tier),
           "ms": {name: {k: stat(name, k) for k in ("read", "text")} for name in runs},
           "device_kernel_ms": {k: stat("device", k, 1.0) for k in ("lines_ms", "parse_ms", "rewrite_ms")},
           "n_host_lines": runs["device"][0]["n_host_lines"]}
    both = {name: statistics.median(r["read"] + r["text"] for r in runs[name]) * 1e3 for name in runs}
    spreads = {name: (max(r["read"] + r["text"] for r in runs[name]) - min(r["read"] + r["text"] for r in runs[name])) * 1e3 for name in runs}
    res["read_plus_text_ms"] = {name: dict(median=both[name], spread=spreads[name]) for name in runs}
    res["device_shorter_by_ms"] = both["parent"] - both["device"]
    res["shorter_by_more_than_both_spreads"] = bool(res["device_shorter_by_ms"] > spreads["parent"] + spreads["device"])
    k_ms = sum(res["device_kernel_ms"][k]["median"] for k in res["device_kernel_ms"])
    res["kernel_share_of_device_read_plus_text"] = k_ms / both["device"]
    parse_s = (res["device_kernel_ms"]["lines_ms"]["median"] + res["device_kernel_ms"]["parse_ms"]["median"]) * 1e-3
    # the plain figure: bytes of the text over the time of lines + parse.  The kernels read the text more than once (vt_lines twice: count and
    # emit; vt_parse once and the INFO / ALT spans again), so the traffic is about three times that: reported beside it, under a name that says so
    res["parse_text_bytes_per_s"] = len(data) / parse_s if parse_s > 0 else None
    res["parse_text_share_of_hbm_copy_rate"] = res["parse_text_bytes_per_s"] / HBM_COPY_BYTES_PER_S if parse_s > 0 else None
    res["parse_traffic_bytes_per_s_assuming_3_reads_of_the_text"] = 3 * len(data) / parse_s if parse_s > 0 else None
    res["host_ms_left_in_device_path"] = both["device"] - k_ms
    say(json.dumps(res))
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(out_lines) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=0, help="N: measure the two text stages on a synthetic cohort-shaped target VCF of N records instead")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--scale", type=float, default=1.0, help="contig lengths of the sample relative to gen_sample's default")
    ap.add_argument("--host-tier", action="store_true", help="plumbing check on the test suite's host build of the kernels (never a measurement)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.targets:
        return targets_bench(a)
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
