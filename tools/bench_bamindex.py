"""The BAM index on the device and the fetch through it, against the whole-file load.

    python tools/bench_bamindex.py [--reads 1500] [--steps 3] [--run-mb 4] > profiles/bamindex_bench.json

The synthetic ONT-like records of tools/bench_bgzf.py (synth_bam.gen_records, 20-kb reads), spread over three contigs and sorted,
BGZF-compressed at level 6.  In one session:
  index   bam.index_bam in runs of --run-mb compressed megabytes: the kernel times (HIP events) of the inflate, the chain and the
          three index stages, and inflated bytes per second through the index kernels
  sample  pipeline.call_sample(..., objects=False) alternating between bam.read_bam_device (the whole file resident) and
          bam.open_indexed (one contig resident at a time): wall time, bytes over PCIe for the input, peak resident stream bytes
One JSON line.  The two samples' VCF texts are compared."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1500)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--run-mb", type=float, default=4.0)
    a = ap.parse_args()
    import struct
    from sniffles_amd import bam, bamindex, pipeline, synth_bam
    from sniffles_amd.config import SnifflesConfig
    names, lens = ["chrA", "chrB", "chrC", "chrD_alt"], [20_000_000, 20_000_000, 20_000_000, 100000]
    recs = []
    for c in range(3):
        recs += synth_bam.gen_records(2026 + c, a.reads // 3, ref_names=names, ref_lens=lens, contig_index=c, style="ont", read_len_mean=20000,
                                      sa_frac=0.2)[2]
    key = lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xffffffff, struct.unpack_from("<i", r, 8)[0])      # (refID -1 last)
    recs.sort(key=key)
    raw = bam.bam_stream(names, lens, recs)
    data = bam.bgzf_deflate(raw, a.level)
    tmp = tempfile.mkdtemp(prefix="bamindex_bench_")
    path = os.path.join(tmp, "sample.bam")
    with open(path, "wb") as f:
        f.write(data)
    run_bytes = int(a.run_mb * (1 << 20))
    # ---- the index build
    builds = []
    for _ in range(a.steps):
        st = {}
        t0 = time.perf_counter()
        index = bam.index_bam(path, out=path + ".bai", run_bytes=run_bytes, stats=st)
        st["total_s"] = time.perf_counter() - t0
        builds.append(st)
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    ms_index = med(builds, "ms_span") + med(builds, "ms_linear") + med(builds, "ms_runs")
    # ---- a whole sample, alternating
    def config():
        cfg = SnifflesConfig(all_contigs=True)
        return cfg
    rows, texts = dict(whole=[], indexed=[]), {}
    for _ in range(a.steps):
        t0 = time.perf_counter()
        d = bam.read_bam_device(path)
        t1 = time.perf_counter()
        buf = io.StringIO()
        pipeline.call_sample(d, config(), vcf_handle=buf, objects=False)
        t2 = time.perf_counter()
        rows["whole"].append(dict(load_s=t1 - t0, total_s=t2 - t0, pcie_in_bytes=int(d.info["bytes_h2d"] + d.info["bytes_d2h"]),
                                  peak_stream_bytes=int(d.info["stream_len"])))
        d.handle.close()
        texts["whole"] = [ln for ln in buf.getvalue().splitlines() if not ln.startswith("##")]
        t0 = time.perf_counter()
        f = bam.open_indexed(path)
        t1 = time.perf_counter()
        buf = io.StringIO()
        pipeline.call_sample(f, config(), vcf_handle=buf, objects=False)
        t2 = time.perf_counter()
        rows["indexed"].append(dict(load_s=t1 - t0, total_s=t2 - t0, pcie_in_bytes=int(sum(i["bytes_h2d"] + i["bytes_d2h"] for i in f.fetches)),
                                    peak_stream_bytes=int(max(i["stream_len"] for i in f.fetches)), fetches=len(f.fetches),
                                    bytes_read=int(sum(i["bytes_read"] for i in f.fetches))))
        f.close()
        texts["indexed"] = [ln for ln in buf.getvalue().splitlines() if not ln.startswith("##")]
        assert texts["whole"] == texts["indexed"], "the two paths wrote different VCF records"
    out = dict(
        workload=f"{len(recs)} synthetic ONT-like alignment records over 3 contigs, {len(raw) / 1e6:.1f} MB inflated, {len(data) / 1e6:.1f} MB as BGZF "
                 f"(level {a.level}, {int(bam.bgzf_members(data).shape[0])} members)",
        steps=a.steps,
        index=dict(run_bytes=run_bytes, runs=builds[-1]["runs"], total_s=med(builds, "total_s"), ms_inflate=med(builds, "ms_inflate"),
                   ms_chain=med(builds, "ms_chain"), ms_span=med(builds, "ms_span"), ms_linear=med(builds, "ms_linear"), ms_runs=med(builds, "ms_runs"),
                   index_kernels_GBps=len(raw) / (ms_index * 1e6), with_inflate_GBps=len(raw) / ((ms_index + med(builds, "ms_inflate") + med(builds, "ms_chain")) * 1e6),
                   peak_stream_bytes=builds[-1]["peak_stream_len"], bytes_h2d=builds[-1]["bytes_h2d"], bai_bytes=len(bamindex.bai_bytes(index)),
                   mapped=index.mapped),
        whole_file={k: (med(rows["whole"], k) if k.endswith("_s") else rows["whole"][-1][k]) for k in rows["whole"][-1]},
        indexed={k: (med(rows["indexed"], k) if k.endswith("_s") else rows["indexed"][-1][k]) for k in rows["indexed"][-1]},
        vcf_records=len([ln for ln in texts["whole"] if not ln.startswith("#")]))
    out["peak_residency_ratio"] = out["indexed"]["peak_stream_bytes"] / out["whole_file"]["peak_stream_bytes"]
    out["wall_ratio_indexed_over_whole"] = out["indexed"]["total_s"] / out["whole_file"]["total_s"]
    print(json.dumps(out))
    for name in os.listdir(tmp):
        os.unlink(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
