"""The output side of the container layer: BGZF deflate on the device (bgzfout.DeflateDevice, csrc/snf_deflate.h) against what the
reference does on one host thread.

    python tools/bench_deflate.py [--mb 15] [--steps 3] > profiles/deflate_bench.json

Two workloads, both paths alternating in one session:
  vcf   a whole-genome-sized VCF text: the record lines of the tests/golden/vcf_text.json.gz fixtures repeated with shifted positions;
        host: zlib level 6, member by member of 0xff00 bytes (what pysam.tabix_index / bgzip do); device: DeflateDevice.compress
  snf   the pickled blocks of the committed .snf fixtures, repeated to the same size; host: gzip.compress (level 9) block by block (the
        SNF writer); device: all blocks in one run, each cut into members of 0xff00 bytes
One JSON line: the kernel time (HIP events), the wall time of compress() with both copies, GB/s of input, the compressed sizes beside
zlib levels 1 and 6 on the same member cuts."""
import argparse
import gzip
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def vcf_text(target: int) -> bytes:
    with gzip.open(os.path.join(GOLDEN, "vcf_text.json.gz")) as f:
        doc = json.load(f)
    head, rows = None, []
    for group in ("single", "combine"):
        for name in sorted(doc[group]):
            for kind, text in sorted(doc[group][name]["text"].items()):
                lines = text.split("\n")
                if head is None:
                    head = [ln for ln in lines if ln.startswith("#")]
                rows += [ln.split("\t") for ln in lines if ln and not ln.startswith("#")]
    out, size, shift = ["\n".join(head) + "\n"], 0, 0
    while size < target:
        for f in rows:
            ln = "\t".join([f[0], str(int(f[1]) + shift)] + f[2:]) + "\n"
            out.append(ln)
            size += len(ln)
        shift += 1_000_000
    return "".join(out).encode()


def snf_blocks(target: int) -> list:
    blocks = []
    for name in sorted(os.listdir(GOLDEN)):
        if not name.endswith(".snf"):
            continue
        with open(os.path.join(GOLDEN, name), "rb") as f:
            header, body = f.read().split(b"\n", 1)
        for per_contig in json.loads(header)["index"].values():
            for parts in per_contig.values():
                for off, length in parts:
                    blocks.append(gzip.decompress(body[off:off + length]))
    out, size = [], 0
    while size < target:
        for b in blocks:
            out.append(b)
            size += len(b)
    return out


def zlib_members(data: bytes, cuts, level: int) -> int:
    total, p = 0, 0
    for n in cuts:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(data[p:p + n]) + c.flush()) + 26
        p += n
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=15.0)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    from sniffles_amd import bgzfout
    target = int(a.mb * 1e6)
    text = vcf_text(target)
    blocks = snf_blocks(target)
    blob = b"".join(blocks)
    block_cuts = [c for b in blocks for c in bgzfout.cut_members(len(b))]
    text_cuts = bgzfout.cut_members(len(text))
    z = bgzfout.DeflateDevice(0)
    z.compress(text[:1 << 20])      # (the first launch loads the code object)
    rows = dict(vcf_host=[], vcf_device=[], snf_host=[], snf_device=[])
    sizes = {}
    for _ in range(a.steps):
        t0 = time.perf_counter()
        sizes["vcf_zlib6"] = zlib_members(text, text_cuts, 6)
        rows["vcf_host"].append(dict(wall_s=time.perf_counter() - t0))
        t0 = time.perf_counter()
        image, off = z.compress(text)
        rows["vcf_device"].append(dict(wall_s=time.perf_counter() - t0, ms_kernel=z.ms_kernel))
        sizes["vcf_device"] = len(image)
        t0 = time.perf_counter()
        sizes["snf_gzip9"] = sum(len(gzip.compress(b)) for b in blocks)
        rows["snf_host"].append(dict(wall_s=time.perf_counter() - t0))
        t0 = time.perf_counter()
        image2, off2 = z.compress(blob, block_cuts)
        rows["snf_device"].append(dict(wall_s=time.perf_counter() - t0, ms_kernel=z.ms_kernel))
        sizes["snf_device"] = len(image2)
    assert gzip.decompress(image) == text and gzip.decompress(image2) == blob
    z.close()
    sizes["vcf_zlib1"] = zlib_members(text, text_cuts, 1)
    sizes["snf_zlib1"] = zlib_members(blob, block_cuts, 1)
    sizes["snf_zlib6"] = zlib_members(blob, block_cuts, 6)
    med = lambda k, f: float(np.median([r[f] for r in rows[k]]))

    def side(kind, n_in, host, cuts):
        dev = kind + "_device"
        return dict(input_bytes=n_in, members=len(cuts), host_wall_s=med(host, "wall_s"), host_GBps=n_in / med(host, "wall_s") / 1e9,
                    device_wall_s=med(dev, "wall_s"), device_wall_GBps=n_in / med(dev, "wall_s") / 1e9, ms_kernel=med(dev, "ms_kernel"),
                    kernel_GBps=n_in / (med(dev, "ms_kernel") * 1e6), wall_speedup=med(host, "wall_s") / med(dev, "wall_s"))
    out = dict(workload=f"{len(text) / 1e6:.1f} MB of VCF text ({len(text_cuts)} members); {len(blob) / 1e6:.1f} MB of pickled SNF blocks "
                        f"({len(blocks)} blocks, {len(block_cuts)} members)", steps=a.steps,
               vcf=side("vcf", len(text), "vcf_host", text_cuts), snf=side("snf", len(blob), "snf_host", block_cuts),
               compressed_bytes=sizes,
               ratio=dict(vcf_device=sizes["vcf_device"] / len(text), vcf_zlib1=sizes["vcf_zlib1"] / len(text), vcf_zlib6=sizes["vcf_zlib6"] / len(text),
                          snf_device=sizes["snf_device"] / len(blob), snf_zlib1=sizes["snf_zlib1"] / len(blob), snf_zlib6=sizes["snf_zlib6"] / len(blob),
                          snf_gzip9=sizes["snf_gzip9"] / len(blob)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
