"""Reference FASTA access for the two places the path reads reference bases: `LeadProvider._mask_N_coverage`
(`src/sniffles/leadprov.py:420-443`: coverage reads as 0 where the reference base is 'N') and the VCF writer's REF / ALT
resolution (`vcf.py:108-120, 302-342`).  The reference opens `pysam.FastaFile(config.reference)`; pysam is not part of this
package, so this is a plain reader with pysam's `fetch(contig[, start, end]) -> str` contract: an existing `.fai` index is
used (offset / line-bases / line-width arithmetic, one `seek` per fetch; for gzip input the offsets index the decompressed text),
otherwise the text is scanned once - one vectorised pass over its newlines - to build the same table in memory.  Plain-text FASTA
and gzip (read fully, once) are served; bgzip random access is container I/O this package
leaves to the caller (any object with `fetch` can be handed to `pipeline.call_sample(reference=...)` instead).
`FastaFile` is host-side container I/O only: nothing in it computes.

`open_device(path)` is the opt-in, device-resident form (`DeviceFasta`, csrc/snf_fasta.h): the whole text in HBM - a bgzip file is
inflated there by the BGZF kernels, run by run -, the `.fai` table built on the device when no `.fai` lies beside the file, the runs
of 'N' of a region (`nmask`) and batched fetches (`fetch_many`) computed where the text is.  `FastaFile` stays the default and the
comparator of every test of the device form."""
from __future__ import annotations

import gzip
import io
import os
import struct


class FastaFile:
    def __init__(self, path: str):
        self.path = path
        self._index = {}          # contig -> (length, offset, line_bases, line_width)
        self._mem = None          # gzip input: the decompressed bytes
        with open(path, "rb") as f:
            gz = f.read(2) == b"\x1f\x8b"
        fai = path + ".fai"
        if os.path.exists(fai):       # (offsets of the UNCOMPRESSED text: they index the decompressed buffer of a gzip / bgzip file just as well)
            with open(fai) as f:
                for line in f:
                    p = line.rstrip("\n").split("\t")
                    if len(p) >= 5:
                        self._index[p[0]] = (int(p[1]), int(p[2]), int(p[3]), int(p[4]))
        if gz:
            with gzip.open(path, "rb") as f:
                self._mem = f.read()
            if not self._index:
                self._scan_bytes(self._mem)
        elif not self._index:
            with open(path, "rb") as f:
                self._scan_bytes(f.read())
        self.references = list(self._index)
        self._handle = None

    def _scan_bytes(self, data: bytes) -> None:
        """The `.fai` table of a FASTA text held in memory: one vectorised pass over the newline positions (a human reference has
        ~50 M lines: a Python loop per line took minutes), per record the name, the offset of its first base, the bases and bytes of
        its first sequence line and the number of bases (all sequence lines but the last have the first line's width, as `faidx`
        requires)."""
        import numpy as np
        buf = np.frombuffer(data, np.uint8)
        n = len(buf)
        if n == 0:
            return
        nl = np.flatnonzero(buf == 10)
        starts = np.concatenate(([0], nl + 1))
        starts = starts[starts < n]                               # first byte of every line
        ends = np.concatenate((nl, [n]))[:len(starts)]            # its newline (or the end of the text)
        hdr = np.flatnonzero(buf[starts] == ord(">"))
        for k, h in enumerate(hdr):
            first, last = h + 1, (hdr[k + 1] if k + 1 < len(hdr) else len(starts))      # sequence lines of this record: [first, last)
            head = bytes(data[starts[h] + 1:ends[h]])
            name = head.split()[0].decode("ascii") if head.split() else ""
            if first >= last:
                self._index[name] = (0, int(ends[h]) + 1, 1, 1)
                continue
            ls, le = starts[first:last], ends[first:last]
            cr = (buf[np.maximum(le - 1, ls)] == 13) & (le > ls)  # "\r\n" line ends
            bases = (le - ls) - cr
            lb = int(bases[0]); lw = int((le[0] - ls[0]) + (1 if le[0] < n else 0))
            self._index[name] = (int(bases.sum()), int(ls[0]), lb or 1, lw or 1)

    def get_reference_length(self, contig: str) -> int:
        return self._index[contig][0]

    def fetch(self, contig, start=None, end=None) -> str:
        """pysam semantics: unknown contig -> KeyError; start / end clipped to the contig; start > end -> ValueError."""
        if contig not in self._index:
            raise KeyError(f"sequence '{contig}' not present")
        length, offset, lb, lw = self._index[contig]
        start = 0 if start is None else int(start)
        end = length if end is None else min(int(end), length)
        if start < 0:
            raise ValueError(f"start out of range ({start})")
        if start > end:
            if start >= length:
                return ""
            raise ValueError(f"invalid coordinates: start ({start}) > stop ({end})")
        if start == end:
            return ""
        b0 = offset + (start // lb) * lw + start % lb
        b1 = offset + ((end - 1) // lb) * lw + (end - 1) % lb + 1
        if self._mem is not None:
            raw = self._mem[b0:b1]
        else:
            if self._handle is None:
                self._handle = open(self.path, "rb")
            self._handle.seek(b0)
            raw = self._handle.read(b1 - b0)
        return raw.replace(b"\n", b"").replace(b"\r", b"").decode("ascii")

    def close(self) -> None:
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def read_fai(path: str) -> dict:
    """The table of `path`.fai as `FastaFile` reads it (lines of fewer than five columns are skipped); {} when there is no such file."""
    index = {}
    fai = path + ".fai"
    if os.path.exists(fai):
        with open(fai) as f:
            for line in f:
                p = line.rstrip("\n").split("\t")
                if len(p) >= 5:
                    index[p[0]] = (int(p[1]), int(p[2]), int(p[3]), int(p[4]))
    return index


def _is_bgzf(head: bytes) -> bool:
    """gzip magic, FEXTRA, and a BC subfield of two bytes in the first member's extra field."""
    if len(head) < 18 or head[:4] != b"\x1f\x8b\x08\x04":
        return False
    xlen = struct.unpack_from("<H", head, 10)[0]
    q = 12
    while q + 4 <= min(12 + xlen, len(head)):
        slen = struct.unpack_from("<H", head, q + 2)[0]
        if head[q] == 66 and head[q + 1] == 67 and slen == 2:
            return True
        q += 4 + slen
    return False


class DeviceFasta:
    """A reference FASTA whose text lives in HBM (one `snf_fasta_t`).  `references`, `get_reference_length` and `fetch` are
    `FastaFile`'s - same values, same exceptions -, so the object stands wherever a reference handle stands; `fetch_many` and `nmask`
    are what the device form adds.  Built by `open_device`."""

    def __init__(self, path: str, device: int = 0, run_bytes: int = 256 << 20):
        import ctypes as C
        import time
        import numpy as np
        from . import abi, bam, lib as L
        self.path, self.device = path, device
        self.lib = L.load()
        self._err = L.SnifflesAmdError
        self._h = C.c_void_p()
        self.timing = dict(read_s=0.0, upload_s=0.0, inflate_ms=0.0, index_ms=0.0, runs=0)
        t0 = time.perf_counter()
        with open(path, "rb") as f:
            data = f.read()
        gz = data[:2] == b"\x1f\x8b"
        bgzf = gz and _is_bgzf(data[:65536])
        mem = None
        if bgzf:
            mem = bam.bgzf_members(data)
            total = int(mem["isize"].sum())
        elif gz:
            data = gzip.decompress(data)
            total = len(data)
        else:
            total = len(data)
        self.timing["read_s"] = time.perf_counter() - t0
        if self.lib.snf_fasta_create(device, total, C.byref(self._h)) != 0:
            self._h = C.c_void_p()
            self._raise()
        try:
            t0 = time.perf_counter()
            buf = np.frombuffer(data, np.uint8)
            if bgzf:
                k, n_mem = 0, int(mem.shape[0])
                ends = mem["payload_off"] + mem["payload_len"].astype(np.int64)      # (the kernels read the payloads only: a run is cut there)
                while k < n_mem:
                    j = k + 1
                    lo = int(mem["payload_off"][k])
                    while j < n_mem and int(ends[j]) - lo <= int(run_bytes):
                        j += 1
                    run = np.ascontiguousarray(mem[k:j]).copy()
                    hi = int(run["payload_off"][-1]) + int(run["payload_len"][-1])
                    run["payload_off"] -= lo
                    run["out_off"] -= run["out_off"][0]
                    piece = buf[lo:hi]
                    ms = C.c_float()
                    self._check(self.lib.snf_fasta_load_bgzf(self._h, piece.ctypes.data if piece.shape[0] else None, int(piece.shape[0]),
                                                             run.ctypes.data, int(run.shape[0]), C.byref(ms)))
                    self.timing["inflate_ms"] += float(ms.value)
                    self.timing["runs"] += 1
                    k = j
            else:
                self._check(self.lib.snf_fasta_load_text(self._h, buf.ctypes.data if total else None, total))
                self.timing["runs"] = 1
            self.timing["upload_s"] = time.perf_counter() - t0
            self.text_len = total
            self._index = read_fai(path)          # contig -> (length, offset, line_bases, line_width), as FastaFile._index
            if not self._index:
                self._index = self._device_index()
            self.references = list(self._index)
            self._ids = {name: i for i, name in enumerate(self.references)}
            tab = np.array([self._index[n] for n in self.references], np.int64).reshape(-1, 4)
            cols = [np.ascontiguousarray(tab[:, c]) for c in range(4)]
            self._check(self.lib.snf_fasta_set_index(self._h, len(self.references), *[c.ctypes.data if len(c) else None for c in cols]))
        except Exception:
            self.close()
            raise

    # ---- plumbing
    def _raise(self):
        raise self._err(self.lib.snf_fasta_last_error().decode("utf-8", "replace"))

    def _check(self, rc):
        if rc != 0:
            self._raise()

    def _device_index(self) -> dict:
        """`FastaFile._scan_bytes` from what fa_index sends back: per header line its byte range, the first sequence line and the
        counts of line ends of the record's span."""
        import ctypes as C
        import numpy as np
        from . import abi
        r = abi.snf_fasta_index_result_t()
        self._check(self.lib.snf_fasta_index(self._h, C.byref(r)))
        self.timing["index_ms"] = float(r.ms_kernel)
        n, text_len = int(r.n_records), int(r.text_len)
        index = {}
        if not n:
            return index
        rec = np.ctypeslib.as_array(C.cast(r.rec, C.POINTER(C.c_uint8)), shape=(n * abi.FASTA_RECORD_DTYPE.itemsize,)).view(abi.FASTA_RECORD_DTYPE).copy()
        hoff = np.ctypeslib.as_array(r.header_off, shape=(n + 1,)).copy()
        heads = np.ctypeslib.as_array(r.headers, shape=(max(1, int(hoff[-1])),)).tobytes()
        for k in range(n):
            head = heads[int(hoff[k]) + 1:int(hoff[k + 1])].split()
            name = head[0].decode("ascii") if head else ""
            ls, le, se = int(rec["line_start"][k]), int(rec["line_end"][k]), int(rec["span_end"][k])
            if ls >= se:
                index[name] = (0, int(rec["header_end"][k]) + 1, 1, 1)
                continue
            bases = (se - ls) - int(rec["n_newline"][k]) - int(rec["n_cr"][k])
            lb = (le - ls) - int(rec["line_cr"][k])
            lw = (le - ls) + (1 if le < text_len else 0)
            index[name] = (bases, ls, lb or 1, lw or 1)
        return index

    # ---- FastaFile's interface
    def get_reference_length(self, contig: str) -> int:
        return self._index[contig][0]

    def fetch(self, contig, start=None, end=None) -> str:
        """`FastaFile.fetch`: the same string, the same exceptions."""
        from . import abi
        if contig not in self._index:
            raise KeyError(f"sequence '{contig}' not present")
        length = self._index[contig][0]
        start = 0 if start is None else int(start)
        end = length if end is None else min(int(end), length)
        pool, off, status, _ = self.fetch_many(contig, [start], [end])
        if status[0] == abi.FASTA_START_NEGATIVE:
            raise ValueError(f"start out of range ({start})")
        if status[0] == abi.FASTA_START_ABOVE_END:
            raise ValueError(f"invalid coordinates: start ({start}) > stop ({end})")
        return pool.tobytes().decode("ascii")

    def fetch_many(self, contig, starts, ends):
        """A batch of `fetch(contig, start, end)` in one launch: (pool uint8 - the sequences one behind the other -, off int64[n + 1],
        status int32[n] - abi.FASTA_OK / FASTA_START_NEGATIVE / FASTA_START_ABOVE_END (the two ValueErrors) / FASTA_KEY_ERROR -,
        n_count int32[n] - the bytes 'N' of every sequence)."""
        import ctypes as C
        import numpy as np
        from . import abi
        lim = 1 << 62

        def col(x):
            if isinstance(x, np.ndarray) and x.dtype.kind in "iu" and x.dtype.itemsize <= 8 and x.dtype != np.uint64:
                return np.ascontiguousarray(x, np.int64).reshape(-1)
            return np.array([max(-lim, min(lim, int(v))) for v in x], np.int64)
        s, e = col(starts), col(ends)
        if s.shape != e.shape:
            raise ValueError("fetch_many: starts and ends differ in length")
        n = int(s.shape[0])
        r = abi.snf_fasta_fetch_t()
        self._check(self.lib.snf_fasta_fetch(self._h, self._ids.get(contig, -1), n, s.ctypes.data if n else None, e.ctypes.data if n else None, C.byref(r)))
        self.last_ms = float(r.ms_kernel)
        off = np.ctypeslib.as_array(r.off, shape=(n + 1,)).copy()
        total = int(off[-1])
        pool = np.ctypeslib.as_array(r.pool, shape=(total,)).copy() if total else np.zeros(0, np.uint8)
        status = np.ctypeslib.as_array(r.status, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        n_count = np.ctypeslib.as_array(r.n_count, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return pool, off, status, n_count

    def nruns(self, contig: str, lo: int, hi: int):
        """The runs of 'N' of the bases [lo, hi) of a contig, 0 <= lo <= hi <= length: (start[], end[]) int32, sorted and disjoint - or
        None when the text range did not hold hi - lo bases (lines of another width than the index says)."""
        import ctypes as C
        import numpy as np
        from . import abi
        r = abi.snf_fasta_runs_t()
        self._check(self.lib.snf_fasta_nruns(self._h, self._ids[contig], int(lo), int(hi), C.byref(r)))
        self.last_ms = float(r.ms_kernel)
        if not r.regular:
            return None
        k = int(r.n_runs)
        if not k:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        return np.ctypeslib.as_array(r.start, shape=(k,)).copy(), np.ctypeslib.as_array(r.end, shape=(k,)).copy()

    def _fetch_text_range(self, contig, start=None, end=None) -> str:
        """`FastaFile.fetch` to the letter - the text between the first and the last base's offsets with the line ends taken out -
        through `read_text`: what `nmask` falls back to when a contig's lines are not of one width (no faidx-valid file; `fetch` /
        `fetch_many` address every base by line and column and expect regular lines, as `faidx` does)."""
        if contig not in self._index:
            raise KeyError(f"sequence '{contig}' not present")
        length, offset, lb, lw = self._index[contig]
        start = 0 if start is None else int(start)
        end = length if end is None else min(int(end), length)
        if start < 0:
            raise ValueError(f"start out of range ({start})")
        if start > end:
            if start >= length:
                return ""
            raise ValueError(f"invalid coordinates: start ({start}) > stop ({end})")
        if start == end:
            return ""
        b0 = offset + (start // lb) * lw + start % lb
        b1 = min(offset + ((end - 1) // lb) * lw + (end - 1) % lb + 1, self.text_len)
        return self.read_text(b0, max(0, b1 - b0)).replace(b"\n", b"").replace(b"\r", b"").decode("ascii")

    def nmask(self, contig: str, regions, contig_len: int):
        """`soa.paint_nmask(FastaFile(path).fetch, contig, regions, contig_len)`: the same arrays, the same exceptions.  The plain
        case - the contig has `contig_len` bases, every region is 0 <= start <= end - takes one fa_nruns call per clipped region and
        paints in list order on the host; everything else (a length mismatch, the one-base broadcast, negative coordinates, an unknown
        contig) goes through `paint_nmask(self.fetch, ...)` and raises what that raises."""
        import numpy as np
        from . import soa
        contig_len = int(contig_len)
        plain = contig in self._index and self._index[contig][0] == contig_len
        if plain and regions is not None:
            regions = [(int(a), int(b)) for a, b in regions]
            plain = all(0 <= a <= b for a, b in regions)
        if not plain:
            return soa.paint_nmask(self.fetch, contig, regions, contig_len)
        if regions is None:
            runs = self.nruns(contig, 0, contig_len)
            return runs if runs is not None else soa.paint_nmask(self._fetch_text_range, contig, None, contig_len)
        cur = []
        for a, b in regions:
            lo, hi = min(a, contig_len), min(b, contig_len)
            if hi <= lo:
                continue
            runs = self.nruns(contig, lo, hi)
            if runs is None:                 # lines of another width than the index says: FastaFile's answer, from the text range
                return soa.paint_nmask(self._fetch_text_range, contig, regions, contig_len)
            cur = soa.paint_region(cur, lo, hi, runs[0], runs[1])
        return np.array([s for s, _ in cur], np.int32), np.array([e for _, e in cur], np.int32)

    def read_text(self, off: int, n: int) -> bytes:
        """Text bytes back to the host (tests)."""
        import numpy as np
        out = np.zeros(max(1, int(n)), np.uint8)
        self._check(self.lib.snf_fasta_read_text(self._h, int(off), int(n), out.ctypes.data))
        return out[:int(n)].tobytes()

    def close(self) -> None:
        if self._h:
            self.lib.snf_fasta_destroy(self._h)
            self._h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def open_device(path: str, device: int = 0, run_bytes: int = 256 << 20) -> DeviceFasta:
    """The reference at `path` resident on `device`: plain text in one upload; a bgzip file (first member BGZF) as its compressed
    bytes, inflated on the device in runs of `run_bytes`; any other gzip file inflated on the host, as `FastaFile` does, and uploaded.
    A `.fai` beside the file is used as `FastaFile` uses it, else the table is built on the device."""
    return DeviceFasta(path, device, run_bytes)
