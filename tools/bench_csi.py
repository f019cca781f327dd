"""The cost of the run-time level loop: bam.index_bam as BAI and as CSI on the file of tools/bench_bamindex.py, alternating.

    python tools/bench_csi.py [--rounds 5] [--steps 5] [--run-mb 4] [--parent DIR] > profiles/csi_bench.json

Every variant of every round is a process of its own (a library is loaded once per process): `bai` and `csi` of this tree and,
with --parent DIR (a checkout of the parent commit with its library built), `parent_bai` from there.  A process builds the index
once unmeasured and then --steps times; per build it prints ms_span, ms_linear, ms_runs (HIP events, summed over the runs of the
file) and, for a CSI, the wall time of bamindex.csi_bytes.  The last line is the summary: median, min and max per variant."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ms_span", "ms_linear", "ms_runs", "ms_csi_bytes", "total_ms")


def child(a):
    sys.path.insert(0, a.root)
    from sniffles_amd import bam, bamindex
    kw = dict(fmt="csi") if a.fmt == "csi" else {}
    for step in range(a.steps + 1):
        st = {}
        t0 = time.perf_counter()
        index = bam.index_bam(a.path, run_bytes=int(a.run_mb * (1 << 20)), stats=st, **kw)
        row = dict(ms_span=st["ms_span"], ms_linear=st["ms_linear"], ms_runs=st["ms_runs"], total_ms=(time.perf_counter() - t0) * 1e3, runs=st["runs"])
        if a.fmt == "csi":
            t0 = time.perf_counter()
            data = bamindex.csi_bytes(index)
            row.update(ms_csi_bytes=(time.perf_counter() - t0) * 1e3, csi_bytes=len(data), depth=index.depth)
        if step:
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=1500)
    ap.add_argument("--run-mb", type=float, default=4.0)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--fmt", default="bai")
    ap.add_argument("--path", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    from sniffles_amd import bam, synth_bam
    names, lens = ["chrA", "chrB", "chrC", "chrD_alt"], [20_000_000, 20_000_000, 20_000_000, 100000]
    recs = []
    for c in range(3):
        recs += synth_bam.gen_records(2026 + c, a.reads // 3, ref_names=names, ref_lens=lens, contig_index=c, style="ont", read_len_mean=20000,
                                      sa_frac=0.2)[2]
    recs.sort(key=lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xffffffff, struct.unpack_from("<i", r, 8)[0]))
    raw = bam.bam_stream(names, lens, recs)
    tmp = tempfile.mkdtemp(prefix="csi_bench_")
    path = os.path.join(tmp, "sample.bam")
    with open(path, "wb") as f:
        f.write(bam.bgzf_deflate(raw, 6))
    variants = ([("parent_bai", a.parent, "bai")] if a.parent else []) + [("bai", ROOT, "bai"), ("csi", ROOT, "csi")]
    rows = {v[0]: [] for v in variants}
    try:
        for rnd in range(a.rounds):
            for name, root, fmt in variants:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--fmt", fmt, "--path", path, "--steps", str(a.steps),
                       "--run-mb", str(a.run_mb)]
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
                for ln in out.splitlines():
                    row = json.loads(ln)
                    rows[name].append(row)
                    print(json.dumps(dict(variant=name, round=rnd, **row)), flush=True)
    finally:
        os.unlink(path)
        os.rmdir(tmp)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    summary = dict(workload=f"{len(recs)} synthetic ONT-like alignment records over 3 contigs, {len(raw) / 1e6:.1f} MB inflated", rounds=a.rounds, steps=a.steps)
    for name in rows:
        summary[name] = {k: dict(median=med(v), min=min(v), max=max(v)) for k in KEYS for v in [[r[k] for r in rows[name] if k in r]] if v}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
