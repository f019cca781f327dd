"""The container layer in front of the extraction, host path against device path, both up to "extraction input resident in HBM".

    python tools/bench_bgzf.py [--reads 1500] [--tile 1] [--steps 3] > profiles/bgzf_bench.json

The synthetic ONT-like BAM of tools/bench_extract.py (synth_bam.gen_records, 20-kb reads), BGZF-compressed at level 6 like
samtools.  In one session, alternating:
  host    bam.bgzf_inflate (zlib, one thread) + bam.parse_bam + bam.contig_records + Extractor.upload (inflated bytes over PCIe)
  device  bam.bam_device (compressed bytes over PCIe; bgzf_inflate_wave, bam_chain, bam_heads) + bam.contig_records (a view) +
          Extractor.upload (snf_extract_attach_device)
One JSON line: wall times of both, the inflate and chain kernel times (HIP events), inflated bytes per second, the bytes that
cross PCIe on both paths, the file's compression ratio, zlib's single-thread rate beside the kernel's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1500)
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    a = ap.parse_args()
    from sniffles_amd import bam, extract, synth_bam
    names, lens, recs = synth_bam.gen_records(2026, a.reads, style="ont", read_len_mean=20000, sa_frac=0.2,
                                              ref_lens=(60_000_000, 300000, 300000, 100000))
    raw = bam.bam_stream(names, lens, recs * a.tile)
    data = bam.bgzf_deflate(raw, a.level)
    n_members = int(bam.bgzf_members(data).shape[0])
    rows = dict(host=[], device=[])
    x = extract.Extractor()
    last = None
    for _ in range(a.steps):
        t0 = time.perf_counter()
        inflated = bam.bgzf_inflate(data)
        t1 = time.perf_counter()
        R = bam.parse_bam(inflated)
        t2 = time.perf_counter()
        C = bam.contig_records(R, "chrA")
        t3 = time.perf_counter()
        x.upload(C, "chrA", 0, 60_000_000)
        t4 = time.perf_counter()
        rows["host"].append(dict(inflate_s=t1 - t0, parse_s=t2 - t1, contig_s=t3 - t2, upload_s=t4 - t3, total_s=t4 - t0,
                                 pcie_bytes=int(C.blob.nbytes + C.rec_off.nbytes + 4 * C.n + 4 * max(1, C.n))))
        assert inflated == raw
        t0 = time.perf_counter()
        D = bam.bam_device(data)
        t1 = time.perf_counter()
        V = bam.contig_records(D, "chrA")
        t2 = time.perf_counter()
        x.upload(V, "chrA", 0, 60_000_000)
        t3 = time.perf_counter()
        i = D.info
        rows["device"].append(dict(read_s=t1 - t0, contig_s=t2 - t1, attach_s=t3 - t2, total_s=t3 - t0, ms_inflate=i["ms_inflate"], ms_chain=i["ms_chain"],
                                   pcie_bytes=int(i["bytes_h2d"] + i["bytes_d2h"] + 8 * (V.n + 1) + 4 * V.n + 4 * max(1, V.n))))
        assert np.array_equal(D.rec_off, R.rec_off) and np.array_equal(D.ref_id, R.ref_id)
        if last is not None:
            last.handle.close()
        last = D
    x.close()
    last.handle.close()
    med = lambda path, k: float(np.median([r[k] for r in rows[path]]))
    ms_inf, ms_chain = med("device", "ms_inflate"), med("device", "ms_chain")
    out = dict(
        workload=f"{len(recs) * a.tile} synthetic ONT-like alignment records, {len(raw) / 1e6:.1f} MB inflated, {len(data) / 1e6:.1f} MB as BGZF "
                 f"(level {a.level}, {n_members} members)",
        compression_ratio=len(raw) / len(data), steps=a.steps,
        host=dict(total_s=med("host", "total_s"), inflate_s=med("host", "inflate_s"), parse_s=med("host", "parse_s"), contig_s=med("host", "contig_s"),
                  upload_s=med("host", "upload_s"), pcie_bytes=rows["host"][-1]["pcie_bytes"],
                  zlib_one_thread_GBps=len(raw) / med("host", "inflate_s") / 1e9),
        device=dict(total_s=med("device", "total_s"), read_s=med("device", "read_s"), contig_s=med("device", "contig_s"), attach_s=med("device", "attach_s"),
                    ms_inflate=ms_inf, ms_chain=ms_chain, inflate_out_GBps=len(raw) / (ms_inf * 1e6), chain_GBps=len(raw) / (ms_chain * 1e6),
                    pcie_bytes=rows["device"][-1]["pcie_bytes"]),
        speedup_to_resident=med("host", "total_s") / med("device", "total_s"))
    out["inflate_kernel_vs_zlib_16_threads"] = out["device"]["inflate_out_GBps"] / (16 * out["host"]["zlib_one_thread_GBps"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
