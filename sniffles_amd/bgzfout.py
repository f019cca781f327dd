"""The output side of the container layer: BGZF members deflated on the GPU (csrc/snf_deflate.h), `.vcf.gz` and its tabix index.

The reference writes `--vcf out.vcf.gz` as text and then calls `pysam.tabix_index(..., preset="vcf", force=True)`
(`sniffles:573-584`): zlib level 6 on one host thread.  Here the text goes through `deflate_member` in runs of members,
and the index (tabix specification, VCF preset) is made from the lines as they pass:

    with bgzfout.VcfGzWriter("out.vcf.gz") as h:
        pipeline.call_sample(records, config, vcf_handle=h)

Everything here is opt-in; a plain text handle and `gzip.compress` stay the defaults of the drivers and of the SNF writer.
"""
from __future__ import annotations

import re
import struct

import numpy as np

from . import bamindex

MEMBER_MAX = 0xff00      # htslib's cut: input bytes of a BGZF member
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class DeflateDevice:
    """One `snf_deflate_t`: compresses runs of BGZF members on the GPU."""

    def __init__(self, device: int = 0):
        import ctypes as C
        from . import lib as L
        self.lib = L.load()
        self._err = L.SnifflesAmdError
        self.device = device
        self.ms_kernel = 0.0      # kernel time of the last run (HIP events)
        self._h = C.c_void_p()
        self._check(self.lib.snf_deflate_create(device, C.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            raise self._err(self.lib.snf_deflate_last_error().decode("utf-8", "replace"))

    def compress(self, data, member_len=None):
        """`member_len`: input bytes of every member (each at most 0xff00, together len(data)); None: cuts of 0xff00 bytes.
        Returns (the members as bytes, int64[n + 1] offsets of the members in them).  No EOF member is appended."""
        import ctypes as C
        from . import abi
        buf = np.frombuffer(data, np.uint8)
        if member_len is None:
            n = (buf.shape[0] + MEMBER_MAX - 1) // MEMBER_MAX
            member_len = np.full(n, MEMBER_MAX, np.uint32)
            if n:
                member_len[-1] = buf.shape[0] - (n - 1) * MEMBER_MAX
        ml = np.asarray(member_len)
        if ml.shape[0] and (int(ml.min()) < 0 or int(ml.max()) > 0xffffffff):
            raise ValueError("a member length outside 0 .. 2^32 - 1")
        ml = np.ascontiguousarray(ml, np.uint32)
        r = abi.snf_deflate_result_t()
        self._check(self.lib.snf_deflate_run(self._h, buf.ctypes.data if buf.shape[0] else None, int(buf.shape[0]),
                                             ml.ctypes.data if ml.shape[0] else None, int(ml.shape[0]), C.byref(r)))
        self.ms_kernel = float(r.ms_kernel)
        image = C.string_at(r.image, r.image_len) if r.image_len else b""
        off = np.ctypeslib.as_array(r.member_off, (int(r.n_members) + 1,)).astype(np.int64)      # (a copy: the library's until the next run)
        return image, off

    def close(self):
        if self._h:
            self.lib.snf_deflate_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def cut_members(length: int) -> list:
    """Member lengths of `length` bytes cut at 0xff00."""
    full, rest = divmod(int(length), MEMBER_MAX)
    return [MEMBER_MAX] * full + ([rest] if rest else [])


class BgzfWriter:
    """A file-like object: `write(str | bytes)`, `close()`.  The bytes are cut into members of 0xff00 bytes, compressed on the
    device in runs of about `run_bytes`, and the 28-byte EOF member ends the file.  `deflater`: a DeflateDevice to share."""

    def __init__(self, path: str, device: int = 0, run_bytes: int = 64 << 20, deflater: DeflateDevice = None):
        self.path = path
        self._own = deflater is None
        self._z = deflater if deflater is not None else DeflateDevice(device)
        self._f = open(path, "wb")
        self._run = max(1, int(run_bytes) // MEMBER_MAX) * MEMBER_MAX
        self._parts, self._pending = [], 0
        self.member_off = [0]      # file offset of every member written so far, and of the next one
        self.closed = False

    def write(self, data) -> int:
        if self.closed:
            raise ValueError("write to a closed BgzfWriter")
        b = data.encode("utf-8") if isinstance(data, str) else bytes(data)
        self._take(b)
        self._parts.append(b)
        self._pending += len(b)
        while self._pending >= self._run:
            self._flush(self._run)
        return len(data)

    def _take(self, b: bytes) -> None:      # (VcfGzWriter reads the lines here)
        pass

    def _flush(self, count: int) -> None:
        buf = b"".join(self._parts)
        head, rest = buf[:count], buf[count:]
        self._parts, self._pending = ([rest] if rest else []), len(rest)
        if not head:
            return
        image, off = self._z.compress(head)
        base = self.member_off[-1]
        self._f.write(image)
        self.member_off.extend((off[1:] + base).tolist())

    def flush(self) -> None:
        pass      # (members are cut at fixed input offsets: nothing is written before a run is full)

    def _finish(self) -> None:
        pass

    def close(self) -> None:
        if self.closed:
            return
        try:
            self._flush(self._pending)
            self._f.write(EOF_MEMBER)
            self.member_off.append(self.member_off[-1] + len(EOF_MEMBER))      # [-2]: where the EOF member starts
            self._f.close()
            self._finish()
        finally:
            self.closed = True
            if not self._f.closed:
                self._f.close()
            if self._own:
                self._z.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_END = re.compile(rb"(?:^|;)END=(\d+)(?:;|$)")
TBI_META_BIN = bamindex.meta_bin(5)


def vcf_interval(line: bytes, number: int, tbi: bool = True):
    """(contig, beg, end) of a VCF record line as tabix's VCF preset takes it: beg = POS - 1, end = beg + len(REF), an INFO END=
    greater than beg instead.  `tbi`: refuse what a `.tbi` cannot reach (a `.csi` has as many levels as the positions need)."""
    f = line.split(b"\t", 8)
    if len(f) < 8:
        raise ValueError(f"VCF line {number}: {len(f)} columns, a record has at least 8")
    try:
        beg = int(f[1]) - 1
    except ValueError:
        raise ValueError(f"VCF line {number}: POS {f[1][:20]!r} is not a number") from None
    beg = max(beg, 0)
    end = beg + len(f[3])
    m = _END.search(f[7].rstrip(b"\r\n"))
    if m and int(m.group(1)) > beg:
        end = int(m.group(1))
    end = max(end, beg + 1)
    if tbi and end > 1 << 29:
        raise ValueError(f"VCF line {number}: position {end} is beyond 2^29, the last base a tabix index reaches")
    return f[0], beg, end


class VcfGzWriter(BgzfWriter):
    """A BgzfWriter for VCF text that writes `path + ".tbi"` on close().  Usable as the `vcf_handle` of pipeline.call_sample /
    combine / genotype_vcf.  The records must be sorted: a position that decreases inside a contig, or a contig that returns
    after another one, is a ValueError naming the line (the reference refuses `.gz` with `--no-sort` for this reason).
    `index="csi"` writes `path + ".csi"` instead - tabix over CSIv1 (what `pysam.tabix_index(csi=True)` writes), min_shift 14,
    at least 5 levels and as many as the largest end needs: positions beyond 2^29 are accepted."""

    def __init__(self, path: str, device: int = 0, run_bytes: int = 64 << 20, deflater: DeflateDevice = None, index: str = "tbi"):
        if index not in ("tbi", "csi"):
            raise ValueError(f"VcfGzWriter: index {index!r} is neither 'tbi' nor 'csi'")
        super().__init__(path, device, run_bytes, deflater)
        self.index = index
        self._tail = b""
        self._upos = 0           # uncompressed offset of the start of the pending line
        self._line = 0
        self._names, self._seen = [], {}
        self._rec = []           # (contig index, beg, end, uncompressed start, uncompressed end)
        self._last = (-1, -1)

    def _take(self, b: bytes) -> None:
        buf = self._tail + b
        lines = buf.split(b"\n")
        self._tail = lines.pop()
        for ln in lines:
            self._one(ln, len(ln) + 1)

    def _one(self, ln: bytes, size: int) -> None:
        self._line += 1
        start = self._upos
        self._upos += size
        if not ln or ln.startswith(b"#"):
            return
        name, beg, end = vcf_interval(ln, self._line, self.index == "tbi")
        tid = self._seen.get(name)
        if tid is None:
            tid = self._seen[name] = len(self._names)
            self._names.append(name)
        ltid, lbeg = self._last
        if tid != ltid and tid < len(self._names) - 1:
            raise ValueError(f"VCF line {self._line}: contig {name.decode('utf-8', 'replace')} returns after another one - "
                             "a tabix index needs the records of a contig together")
        if tid == ltid and beg < lbeg:
            raise ValueError(f"VCF line {self._line}: position {beg + 1} of {name.decode('utf-8', 'replace')} is below the one before it "
                             f"({lbeg + 1}) - a tabix index needs sorted records")
        self._last = (tid, beg)
        self._rec.append((tid, beg, end, start, self._upos))

    def _voff(self, u: int) -> int:
        return int(self.member_off[u // MEMBER_MAX]) << 16 | (u % MEMBER_MAX)

    def index_bytes(self) -> bytes:
        """The tabix index of what was written (after close())."""
        names = b"".join(n + b"\0" for n in self._names)
        out = [b"TBI\x01", struct.pack("<8i", len(self._names), 2, 1, 2, 0, ord("#"), 0, len(names)), names]
        per = [[] for _ in self._names]
        for r in self._rec:
            per[r[0]].append(r)
        for recs in per:
            bins, order = {}, []
            n_win = ((max(r[2] for r in recs) - 1) >> 14) + 1
            lin = np.full(n_win, bamindex.U64_MAX, np.uint64)
            prev = None
            for _, beg, end, us, ue in recs:
                b = bamindex.reg2bin(beg, end)
                vb, ve = self._voff(us), self._voff(ue)
                if b == prev:
                    bins[b][-1][1] = ve
                else:
                    if b not in bins:
                        bins[b] = []
                        order.append(b)
                    bins[b].append([vb, ve])
                prev = b
                w0, w1 = beg >> 14, (end - 1) >> 14
                lin[w0:w1 + 1] = np.minimum(lin[w0:w1 + 1], np.uint64(vb))
            out.append(struct.pack("<i", len(bins) + 1))
            for b in sorted(bins):
                ch = np.array(bins[b], "<u8")
                out += [struct.pack("<Ii", b, ch.shape[0]), ch.tobytes()]
            out.append(struct.pack("<Ii4Q", TBI_META_BIN, 2, self._voff(recs[0][3]), self._voff(recs[-1][4]), len(recs), 0))
            lin = bamindex.fill_linear(lin)
            out += [struct.pack("<i", lin.shape[0]), lin.astype("<u8").tobytes()]
        out.append(struct.pack("<Q", 0))      # n_no_coor
        return b"".join(out)

    def csi_index(self) -> bamindex.BamIndex:
        """The index of what was written (after close()) as tabix over CSI: the intervals and virtual offsets of `index_bytes`,
        bins of min_shift 14 and the depth the largest end needs (at least 5), the bins' loffset by htslib's rule
        (`bamindex.csi_loffsets`), the tabix header of the VCF preset and the names as the aux block."""
        names = b"".join(n + b"\0" for n in self._names)
        depth, top = 5, max([r[2] for r in self._rec] + [0])
        while top > 1 << (14 + 3 * depth):
            depth += 1
        per = [[] for _ in self._names]
        for r in self._rec:
            per[r[0]].append(r)
        refs = []
        for recs in per:
            bins, prev = {}, None
            lin = np.full(((max(r[2] for r in recs) - 1) >> 14) + 1, bamindex.U64_MAX, np.uint64)
            for _, beg, end, us, ue in recs:
                b = bamindex.reg2bin(beg, end, 14, depth)
                vb, ve = self._voff(us), self._voff(ue)
                if b == prev:
                    bins[b][-1][1] = ve
                else:
                    bins.setdefault(b, []).append([vb, ve])
                prev = b
                w0, w1 = beg >> 14, (end - 1) >> 14
                lin[w0:w1 + 1] = np.minimum(lin[w0:w1 + 1], np.uint64(vb))
            bins = {b: np.array(ch, np.uint64) for b, ch in bins.items()}
            refs.append(bamindex.RefIndex(bins=bins, loffset=bamindex.csi_loffsets(bins, bamindex.fill_linear(lin), depth),
                                          meta=(self._voff(recs[0][3]), self._voff(recs[-1][4]), len(recs), 0)))
        aux = struct.pack("<7i", 2, 1, 2, 0, ord("#"), 0, len(names)) + names
        return bamindex.BamIndex(refs, 0, "csi", 14, depth, aux)

    def _finish(self) -> None:
        if self._tail:      # (a last line without its newline)
            self._one(self._tail, len(self._tail))
            self._tail = b""
        if self.index == "csi":
            bamindex.write_csi(self.csi_index(), self.path + ".csi", deflater=self._z)
            return
        raw = self.index_bytes()
        image, _ = self._z.compress(raw)
        with open(self.path + ".tbi", "wb") as f:
            f.write(image + EOF_MEMBER)
