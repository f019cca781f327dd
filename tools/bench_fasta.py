"""The reference FASTA on the host (fasta.FastaFile, the parent's path) against the device-resident one (fasta.open_device,
csrc/snf_fasta.h).

    python tools/bench_fasta.py [--mb 64] [--steps 3]          # writes profiles/fasta_bench.json

The driver runs every leg as a child process under its own `timeout` and stops at the first one that fails; a leg runs both paths
alternating in one session and reports medians of `--steps` rounds.
  reference   a synthetic reference of about --mb MB in four contigs, 60-base lines, N blocks at the contig ends and in the middle,
              as plain text and as BGZF.  Host: FastaFile open (the `.fai` scan), soa.paint_nmask per contig, 20 000 fetch calls (one
              base, or 50 to 5 000 bases).  Device: open_device with read / upload / inflate / index listed separately (paid once per
              sample), nmask per contig, the same 20 000 queries as one fetch_many; kernel times from HIP events.
  end_to_end  pipeline.call_sample(objects=False) on the two-contig test sample with a FastaFile (the object path: one fetch per call)
              and with a DeviceFasta (the record-table writer, two fetch_many per contig)."""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = (("reference", 900), ("end_to_end", 600))      # (leg, seconds it may take)


def synthetic_reference(mb: float) -> bytes:
    rng = np.random.default_rng(1)
    out = []
    for k, share in enumerate((0.4, 0.3, 0.2, 0.1)):
        n = int(mb * 1e6 * share)
        a = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
        a[:10_000] = 78
        a[n - 10_000:] = 78                              # telomeres
        a[n // 2:n // 2 + n // 50] = 78                  # a centromere of 2 %
        for s in rng.integers(0, n - 2000, 40):          # short gaps
            a[s:s + int(rng.integers(1, 2000))] = 78
        lines = np.full(n + (n + 59) // 60, 10, np.uint8)
        lines[np.arange(n) + np.arange(n) // 60] = a
        out.append(f">chr{k + 1} synthetic\n".encode() + lines.tobytes())
    return b"".join(out)


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def leg_reference(a):
    from sniffles_amd import bam, fasta, soa
    text = synthetic_reference(a.mb)
    tmp = tempfile.mkdtemp()
    paths = {"plain": os.path.join(tmp, "ref.fa"), "bgzf": os.path.join(tmp, "ref.fa.gz")}
    with open(paths["plain"], "wb") as f:
        f.write(text)
    with open(paths["bgzf"], "wb") as f:
        f.write(bam.bgzf_deflate(text))
    rng = np.random.default_rng(2)
    with fasta.open_device(paths["plain"]) as warm:      # (the first launches load the code object)
        warm.nmask(warm.references[0], None, warm.get_reference_length(warm.references[0]))
        warm.fetch_many(warm.references[0], [0], [100])
    out = dict(text_bytes=len(text), steps=a.steps)
    for form, path in paths.items():
        rows = []
        for _ in range(a.steps):
            r = {}
            t0 = time.perf_counter()
            host = fasta.FastaFile(path)
            r["host_open_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            dev = fasta.open_device(path)
            r["device_open_s"] = time.perf_counter() - t0
            r.update({"device_" + k: v for k, v in dev.timing.items()})
            contig = host.references[0]
            length = host.get_reference_length(contig)
            starts = rng.integers(0, length - 5000, 20_000)
            ends = starts + np.where(rng.random(20_000) < 0.5, 1, rng.integers(50, 5000, 20_000))
            t0 = time.perf_counter()
            want_mask = {c: soa.paint_nmask(host.fetch, c, [(0, host.get_reference_length(c) - 1)], host.get_reference_length(c)) for c in host.references}
            r["host_nmask_s"] = time.perf_counter() - t0
            t0, ms = time.perf_counter(), 0.0
            got_mask = {}
            for c in host.references:
                got_mask[c] = dev.nmask(c, [(0, host.get_reference_length(c) - 1)], host.get_reference_length(c))
                ms += dev.last_ms
            r["device_nmask_s"], r["device_nmask_kernel_ms"] = time.perf_counter() - t0, ms
            t0 = time.perf_counter()
            want = [host.fetch(contig, int(s), int(e)) for s, e in zip(starts, ends)]
            r["host_fetch_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            pool, off, status, n_count = dev.fetch_many(contig, starts, ends)
            r["device_fetch_s"], r["device_fetch_kernel_ms"] = time.perf_counter() - t0, dev.last_ms
            assert pool.tobytes() == "".join(want).encode() and not status.any() and int(n_count.sum()) == sum(w.count("N") for w in want)
            for c in host.references:
                assert np.array_equal(got_mask[c][0], want_mask[c][0]) and np.array_equal(got_mask[c][1], want_mask[c][1])
            r["fetched_bytes"] = int(off[-1])
            r["n_intervals"] = int(sum(len(v[0]) for v in want_mask.values()))
            dev.close()
            host.close()
            rows.append(r)
        out[form] = {k: med(rows, k) for k in rows[0]}
        out[form]["file_bytes"] = os.path.getsize(path)
    return out


def leg_end_to_end(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cases
    import vcf_util as vu
    from sniffles_amd import fasta, pipeline
    from sniffles_amd.config import SnifflesConfig
    build, args = cases.SAMPLES["sample_two_contigs_12x"]
    assert not args or all(isinstance(x, str) for x in args)
    recs = build()
    rng = np.random.default_rng(11)
    parts = []
    for name, n in zip(recs.ref_names, recs.ref_lens):
        n = int(n)
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
        for s in rng.integers(0, max(1, n - 6000), 12):
            seq[s:s + int(rng.integers(200, 6000))] = 78
        lines = np.full(n + (n + 59) // 60, 10, np.uint8)
        lines[np.arange(n) + np.arange(n) // 60] = seq
        parts.append(f">{name}\n".encode() + lines.tobytes())
    path = os.path.join(tempfile.mkdtemp(), "ref.fa")
    with open(path, "wb") as f:
        f.write(b"".join(parts))

    def config():
        kw, rest = {}, list(args)
        while rest:
            k = rest.pop(0)[2:].replace("-", "_")
            kw[k] = True
            if rest and not rest[0].startswith("--"):
                v = rest.pop(0)
                for conv in (int, float, str):
                    try:
                        kw[k] = conv(v)
                        break
                    except ValueError:
                        pass
        cfg = SnifflesConfig(**kw)
        for k, v in vu.FIXED.items():
            setattr(cfg, k, v)
        return cfg

    def run(reference):
        buf = io.StringIO()
        t0 = time.perf_counter()
        pipeline.call_sample(recs, config(), vcf_handle=buf, tandem_repeats=getattr(recs, "tandem_repeats", None), objects=False, reference=reference)
        return time.perf_counter() - t0, buf.getvalue()
    host = fasta.FastaFile(path)
    dev = fasta.open_device(path)
    run(dev)                                             # (code objects, caches)
    rows, texts = [], set()
    for _ in range(a.steps):
        th, text_h = run(host)
        td, text_d = run(dev)
        texts |= {text_h, text_d}
        rows.append(dict(host_fasta_s=th, device_fasta_s=td))
    assert len(texts) == 1                               # the same characters
    dev.close()
    return dict(sample="sample_two_contigs_12x", records=sum(1 for ln in text_h.split("\n") if ln and ln[0] != "#"), steps=a.steps,
                call_sample_FastaFile_s=med(rows, "host_fasta_s"), call_sample_DeviceFasta_s=med(rows, "device_fasta_s"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=64.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--leg", choices=[n for n, _ in LEGS])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_bench.json"))
    a = ap.parse_args()
    if a.leg:
        print(json.dumps({"reference": leg_reference, "end_to_end": leg_end_to_end}[a.leg](a)))
        return 0
    doc = dict(workload=f"synthetic reference of about {a.mb:g} MB in four contigs, 60-base lines; medians of {a.steps}")
    for leg, limit in LEGS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--mb", str(a.mb), "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"bench_fasta: leg {leg} ended with status {r.returncode}; nothing further is started", file=sys.stderr)
            return r.returncode
        doc[leg] = json.loads(r.stdout.strip().splitlines()[-1])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
