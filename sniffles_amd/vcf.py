"""VCF output: the writer side of the reference's `VCF` class (`src/sniffles/vcf.py:25-350`) -
`VCF(config, handle)`, `write_header(contigs_lengths)`, `write_call(call) -> int`, `format_genotype`, `format_info`.

Pure text formatting of finished `SVCall`s: no kernel and no arithmetic beyond what the reference's writer does to a
call on its way out (END of precise deletions, SVLEN of sequence-resolved insertions, AC / SUPP_VEC over the samples,
the `minsvlen` cut on insertions, REF / ALT resolution against a reference handle, QUAL clamp).  It is here so that
parity can be stated on the VCF line itself - POS, SVLEN, SVTYPE, GT and every other column - and it reproduces the
reference's quirks because a drop-in must: with a reference handle the IUPAC clean-up table is applied to the whole
ALT column (`<INS>` -> `<INN>`, `<DEL>` -> `<NEL>`, `chrY` in a BND ALT -> `chrN`).
`reference_handle` is any object with pysam's `fetch(contig, start, end) -> str` (raising KeyError / ValueError for an
unknown contig / range).  The force-calling side (`--genotype-vcf`, vcf.py:352-481) is here too: `read_svs_iter` (targets
from a VCF), `rewrite_header_genotype`, `rewrite_genotype`.
"""
from __future__ import annotations

from collections import Counter

IUPAC_AMBIGUOUS = "RYSWKMBDHV"
_IUPAC_TO_N = str.maketrans(IUPAC_AMBIGUOUS, "N" * len(IUPAC_AMBIGUOUS))

# ##-lines after the contig table: (section, ID, Number, Type, Description); Number/Type None = not part of the line
_ALT = [("INS", "Insertion"), ("DEL", "Deletion"), ("DUP", "Duplication"), ("INV", "Inversion"),
        ("BND", "Breakend; Translocation")]
_FORMAT = [("GT", "1", "String", "Genotype"), ("GQ", "1", "Integer", "Genotype quality"),
           ("DR", "1", "Integer", "Number of reference reads"), ("DV", "1", "Integer", "Number of variant reads"),
           ("PS", "1", "Integer", "Phase-block, zero if none or not phased"),
           ("ID", "1", "String", "Individual sample SV ID for multi-sample output")]
_FILTER = [
    ("PASS", "All filters passed"), ("GT", "Genotype filter"), ("SUPPORT_MIN", "Minimum read support filter"),
    ("STDEV_POS", "SV Breakpoint standard deviation filter"), ("STDEV_LEN", "SV length standard deviation filter"),
    ("COV_MIN", "Minimum coverage filter"), ("COV_MIN_GT", "Minimum coverage filter (missing genotype)"),
    ("COV_CHANGE_DEL", "Coverage change filter for DEL"), ("COV_CHANGE_DUP", "Coverage change filter for DUP"),
    ("COV_CHANGE_INS", "Coverage change filter for INS"),
    ("COV_CHANGE_FRAC_US", "Coverage fractional change filter: upstream-start"),
    ("COV_CHANGE_FRAC_SC", "Coverage fractional change filter: start-center"),
    ("COV_CHANGE_FRAC_CE", "Coverage fractional change filter: center-end"),
    ("COV_CHANGE_FRAC_ED", "Coverage fractional change filter: end-downstream"),
    ("COV_VAR", "Coverage variance exceeded"), ("MOSAIC_VAF", "Mosaic variant allele fraction filter"),
    ("NOT_MOSAIC_VAF", "Variant allele fraction filter for non-mosaic"), ("ALN_NM", "Length adjusted mismatch filter"),
    ("STRAND_BND", "Strand support filter for BNDs"), ("STRAND", "Strand support filter for germline SVs"),
    ("STRAND_MOSAIC", "Strand support filter for mosaic SVs"), ("SVLEN_MIN", "SV length filter"),
    ("SVLEN_MIN_MOSAIC", "SV length filter for mosaic SVs (min)"), ("SVLEN_MAX_MOSAIC", "SV length filter for mosaic SVs (max)"),
    ("SINGLE_BREAK", "A single break point was detected but not classified as an SV."),
    ("INLINE_SA", "INLINE/CIGAR-based SV is mostly supported by SA reads"),
    ("MOSAIC_SV_CLOSE_EDGE", "For mosaic SVs, the location is close to the end of the read (either end)"),
    ("GT_FAILED", "Sniffles was unable to genotype this call.")]
_SVLENGTHS = ("SVLENGTHS", ".", "Integer", "Lengths of structural variation (all)")
_INFO_HEAD = [("PRECISE", "0", "Flag", "Structural variation with precise breakpoints"),
              ("IMPRECISE", "0", "Flag", "Structural variation with imprecise breakpoints"),
              ("MOSAIC", "0", "Flag", "Structural variation classified as putative mosaic"),
              ("SVLEN", "1", "Integer", "Length of structural variation")]
_INFO_TAIL = [
    ("SVTYPE", "1", "String", "Type of structural variation"), ("CHR2", "1", "String", "Mate chromsome for BND SVs"),
    ("SUPPORT", "1", "Integer", "Number of reads supporting the structural variation"),
    ("SUPPORT_INLINE", "1", "Integer", "Number of reads supporting an INS/DEL SV (non-split events only)"),
    ("SUPPORT_SA", "1", "Integer", "Number of reads supporting a DEL SV through supplementary alignments (split events)"),
    ("SUPPORT_LONG", "1", "Integer", "Number of soft-clipped reads putatively supporting the long insertion SV"),
    ("END", "1", "Integer", "End position of structural variation"),
    ("STDEV_POS", "1", "Float", "Standard deviation of structural variation start position"),
    ("STDEV_LEN", "1", "Float", "Standard deviation of structural variation length"),
    ("COVERAGE", ".", "Float", "Coverages near upstream, start, center, end, downstream of structural variation"),
    ("STRAND", "1", "String", "Strands of supporting reads for structural variant"),
    ("AC", ".", "Integer", "Allele count, summed up over all samples"),
    ("SUPP_VEC", "1", "String", "List of read support for all samples"),
    ("CONSENSUS_SUPPORT", "1", "Integer", "Number of reads that support the generated insertion (INS) consensus sequence"),
    ("RNAMES", ".", "String", "Names of supporting reads (if enabled with --output-rnames)"),
    ("VAF", "1", "Float", "Variant Allele Fraction"),
    ("COVERAGE_VAR", "1", "Float", "Variance of coverage across large events"),
    ("NM", ".", "Float", "Mean number of query alignment length adjusted mismatches of supporting reads"),
    ("PHASE", ".", "String", "Phasing information derived from supporting reads, represented as list of: "
                              "HAPLOTYPE,PHASESET,HAPLOTYPE_SUPPORT,PHASESET_SUPPORT,HAPLOTYPE_FILTER,PHASESET_FILTER"),
    ("LASM", "0", "Flag", "Local assembly used to detect the structural variant")]
_INFO_POPULATION = [("POPULATION_AF", "1", "Float", "Population Allele Frequency"),
                    ("POPULATION_SIZE", "1", "Integer", "Size of genotyped population for this variant")]


def _fast():
    from . import sv
    return sv._load_fast()


def _filters():
    from . import sv
    return sv.FILTERS


def format_info(key, value) -> str:
    """One INFO entry (vcf.py:26-37): floats with three decimals, lists joined, None as '.', True as a bare flag."""
    if isinstance(value, float):
        return f"{key}={value:.3f}"
    if isinstance(value, list):
        return f"{key}={','.join(value)}"
    if value is None:
        value = "."
    if value is True:
        return f"{key}"
    return f"{key}={value}"


def unpack_phase(phase) -> tuple:
    """(haplotype, phase set for the PS column) of a genotype's phase entry (vcf.py:40-51)."""
    if phase is None:
        hp, ps = None, "."
    else:
        try:
            hp, ps = phase
        except TypeError:
            hp, ps = phase, "."
    if ps is None or ps == "NULL":
        ps = "."
    return hp, ps


def format_genotype(gt, is_phased) -> str:
    """A sample column (vcf.py:54-83): 6-tuples come from single-sample calling, 7-tuples (with the per-sample SV id)
    from combine.  Phased notation only for 0/1 and 1/1 with a haplotype; haplotype "1" puts the ALT allele first."""
    a, b, qual, dr, dv, phase = gt[:6]
    hp, ps = unpack_phase(phase)
    sep = "/"
    if is_phased and hp is not None and (a, b) in ((0, 1), (1, 1)):
        sep = "|"
        if hp == "1":
            a, b = b, a
    cols = [f"{a}{sep}{b}", str(qual), str(dr), str(dv)]
    if is_phased:
        cols.append(str(ps))
    if len(gt) != 6:
        cols.append(str(gt[6]))
    return ":".join(cols)


class VCF:
    def __init__(self, config, handle):
        self.config = config
        self.handle = handle
        self.call_count = 0
        self.info_order = ["SVTYPE", "SVLEN", "END", "SUPPORT", "RNAMES", "COVERAGE", "STRAND"]
        if config.qc_nm_measure:
            self.info_order.append("NM")
        if config.dev_emit_sv_lengths:
            self.info_order.append("SVLENGTHS")
        self.default_genotype = config.genotype_none
        self.genotype_format = config.genotype_format
        if config.phase:
            self.genotype_format += ":PS"
        if config.mode == "combine":
            self.genotype_format += ":ID"
            self.default_genotype += ("NULL",)
        self.reference_handle = None
        self.header_str = ""

    # ---- header
    def write_raw(self, text, endl="\n"):
        self.handle.write(text)
        self.handle.write(endl)

    def write_header_line(self, text):
        self.write_raw("##" + text)

    def _typed(self, section, rows):
        for ident, number, typ, desc in rows:
            self.write_header_line(f'{section}=<ID={ident},Number={number},Type={typ},Description="{desc}">')

    def write_header(self, contigs_lengths):
        cfg = self.config
        self.write_header_line("fileformat=VCFv4.2")
        self.write_header_line(f"source={cfg.version}_{cfg.build}")
        self.write_header_line(f'command="{cfg.command}"')
        self.write_header_line(f'fileDate="{cfg.start_date}"')
        for contig, length in contigs_lengths:
            self.write_header_line(f"contig=<ID={contig},length={length}>")
        for ident, desc in _ALT:
            self.write_header_line(f'ALT=<ID={ident},Description="{desc}">')
        self._typed("FORMAT", _FORMAT)
        for ident, desc in _FILTER:
            self.write_header_line(f'FILTER=<ID={ident},Description="{desc}">')
        self._typed("INFO", _INFO_HEAD)
        if cfg.dev_emit_sv_lengths:
            self._typed("INFO", [_SVLENGTHS])
        self._typed("INFO", _INFO_TAIL)
        if cfg.combine_population:
            self._typed("INFO", _INFO_POPULATION)
        samples = "\t".join(sample_id for _, sample_id in cfg.sample_ids_vcf)
        self.write_raw(f"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{samples}")

    # ---- records
    def _sample_columns(self, call):
        """Per-sample genotype strings, allele count and support vector (vcf.py:229-245)."""
        cols, supp, ac = [], [], 0
        phased = self.config.phase
        for internal_id, _ in self.config.sample_ids_vcf:
            gt = call.genotypes.get(internal_id)
            if gt is None:
                cols.append(format_genotype(self.default_genotype, phased))
                supp.append("0")
                continue
            cols.append(format_genotype(gt, phased))
            if gt[0] != "." and gt[4] > 0:
                ac += gt[0] + gt[1]
                supp.append("1")
            else:
                supp.append("0")
        return cols, ac, "".join(supp)

    def _resolve_sequences(self, call) -> bool:
        """REF / ALT against the reference handle (vcf.py:302-342).  False: the call is not emitted (too many N)."""
        cfg = self.config
        ref = self.reference_handle
        if not cfg.symbolic and call.svtype == "DEL" and ref is not None and abs(call.svlen) <= cfg.max_del_seq_len:
            try:   # the deleted bases behind the last reference base before the SV
                call.ref = ref.fetch(call.contig, call.pos - 1, call.pos - call.svlen)
                call.alt = call.ref[0]
            except (KeyError, ValueError):
                call.ref, call.alt = "N", f"<{call.svtype}>"
            else:
                if "N" in call.ref and Counter(call.ref)["N"] / len(call.ref) > cfg.max_unknown_pct:
                    return False
        if cfg.symbolic:
            call.ref = "N"
            if call.svtype != "BND":
                call.alt = f"<{call.svtype}>"
            return True
        if ref is not None and call.ref == "N":
            start = max(0, call.pos - 1)
            try:
                call.ref = ref.fetch(call.contig, start, start + 1)
            except (KeyError, ValueError):
                pass
            else:
                if call.svtype == "INS" and call.alt != "<INS>":
                    call.alt = call.ref + call.alt
                elif call.svtype == "BND" and call.alt != "<BND>":
                    call.alt = (call.ref + call.alt[1:]) if call.alt.startswith("N") else call.alt[:-1] + call.ref
            call.ref = call.ref.translate(_IUPAC_TO_N)
            call.alt = call.alt.translate(_IUPAC_TO_N)   # also hits symbolic ALTs and BND mate names
        return True

    def write_call(self, call) -> int:
        """One record; returns 1 if a line was written.  Mutates the call like the reference's writer does."""
        cfg = self.config
        if call.is_single_break:
            return 0
        pos = call.pos if call.pos > 0 else 1
        end = pos + abs(call.svlen) if (call.precise and call.svtype == "DEL") else call.end

        sample_cols, ac, supp_vec = self._sample_columns(call)
        if len(cfg.sample_ids_vcf) > 1:
            call.set_info("AC", ac)
            call.set_info("SUPP_VEC", supp_vec)
            if int(supp_vec) == 0:
                return 0
            if ac == 0:
                call.filter = "GT"

        if call.svtype == "INS":
            if call.svlen != len(call.alt) and not cfg.symbolic and call.alt != "<INS>":
                call.svlen = len(call.alt)      # SVLEN follows the resolved sequence (before the REF base is prepended)
            if call.svlen < cfg.minsvlen:
                return 0

        bnd = call.svtype == "BND"
        core = {
            "SVTYPE": call.svtype,
            "SVLEN": None if bnd else call.svlen,
            "SVLENGTHS": None if bnd or not call.svlens else ",".join(map(str, call.svlens)),
            "END": None if bnd else end,
            "SUPPORT": call.support,
            "RNAMES": call.rnames if cfg.output_rnames else None,
            "COVERAGE": ",".join(str(c) for c in (call.coverage_upstream, call.coverage_start, call.coverage_center,
                                                  call.coverage_end, call.coverage_downstream)),
            "STRAND": ("+" if call.fwd > 0 else "") + ("-" if call.rev > 0 else ""),
            "NM": call.nm,
        }
        fields = ["PRECISE" if call.precise else "IMPRECISE"]
        vaf = call.get_info("VAF")
        if cfg.mosaic and (vaf if vaf is not None else 0) <= cfg.mosaic_af_max:
            fields.append("MOSAIC")
        fields.extend(format_info(k, core[k]) for k in self.info_order if core[k] is not None)
        fields.extend(format_info(k, call.info[k]) for k in sorted(call.info) if call.info[k] is not None)

        if not self._resolve_sequences(call):
            return 0
        if call.qual is not None:
            call.qual = max(0, min(60, call.qual))
        row = [call.contig, pos, cfg.id_prefix + call.id, call.ref, call.alt, "." if call.qual is None else call.qual,
               call.filter, ";".join(fields), self.genotype_format] + sample_cols
        self.write_raw("\t".join(str(v) for v in row))
        self.call_count += 1
        return 1

    # ---- merged records without the objects
    def can_write_merged(self) -> bool:
        """The group-table writer (`write_merged`) serves the plain multi-sample merge: two or more sample columns in the order of
        `config.snf_input_info`, no reference FASTA attached, no SVLENGTHS, no pair relabelling."""
        cfg = self.config
        ids = [i for i, _ in cfg.sample_ids_vcf]
        return (self.reference_handle is None and cfg.mode == "combine" and len(ids) > 1 and not cfg.dev_emit_sv_lengths
                and not getattr(cfg, "combine_pair_relabel", False) and not getattr(cfg, "combine_consensus", False)
                and ids == [s["internal_id"] for s in cfg.snf_input_info] and _fast() is not None)

    def merged_text_options(self) -> dict:
        cfg = self.config
        return dict(phase=bool(cfg.phase), symbolic=bool(cfg.symbolic), mosaic=bool(cfg.mosaic) and 0 <= cfg.mosaic_af_max,
                    output_rnames=bool(cfg.output_rnames), nm="NM" in self.info_order, minsvlen=int(cfg.minsvlen),
                    genotype_format=self.genotype_format)

    def write_merged(self, part, sort: bool = True) -> int:
        """One task's merged records as `candstore.execute_many(..., text_writer=self)` returned them - `(text, line_off, pos)` - in the
        order `sorted(calls, key=pos)` gives the objects (stable), or as they are.  Returns the number of lines written."""
        import numpy as np
        text, off, pos = part
        if len(pos) == 0:
            return 0
        if not sort or bool((pos[1:] >= pos[:-1]).all()):      # in order already (candstore formats them so): one slice
            n = int(np.count_nonzero(off[1:] > off[:-1]))
            raw = getattr(self.handle, "buffer", None)      # a text file over a binary one (open(path, "w")): the bytes go as they are
            if raw is not None and getattr(self.handle, "encoding", "").lower().replace("-", "") == "utf8":
                self.handle.flush()
                raw.write(memoryview(text)[int(off[0]):int(off[-1])])
            else:
                self.handle.write(str(memoryview(text)[int(off[0]):int(off[-1])], "utf-8"))
            self.call_count += n
            return n
        order = np.argsort(pos, kind="stable")
        n = 0
        out = []
        for k in order.tolist():
            a, b = int(off[k]), int(off[k + 1])
            if b > a:
                out.append(text[a:b])
                n += 1
        self.handle.write(b"".join(out).decode("utf-8"))
        self.call_count += n
        return n

    def can_write_records(self) -> bool:
        """The record-table writer serves the plain single-sample case: no reference FASTA attached (REF / ALT stay "N" /
        the consensus) or one that is resident on the device (`fasta.DeviceFasta`: its bases come as batched fetches; any other handle
        keeps the object path, one `fetch` per call), one sample column, no SVLENGTHS."""
        cfg = self.config
        ref = self.reference_handle
        if ref is not None:
            from .fasta import DeviceFasta
            if not isinstance(ref, DeviceFasta):
                return False
        return (len(cfg.sample_ids_vcf) == 1 and cfg.sample_ids_vcf[0][0] == 0
                and not cfg.dev_emit_sv_lengths and cfg.mode != "combine" and _fast() is not None)

    def write_records(self, res, ti, order) -> int:
        """The records `order` (indices into `res.calls`, output order) of a finalized single-sample batch as VCF lines: the
        text `write_call` produces for the `SVCall` objects of the same records (sv.materialize_candidates + apply_final),
        formatted straight from the record table by the C extension.  Returns the number of lines written."""
        import numpy as np
        cfg = self.config
        opts = dict(id_prefix=cfg.id_prefix, mosaic=bool(cfg.mosaic), mosaic_af_max=float(cfg.mosaic_af_max),
                    output_rnames=bool(cfg.output_rnames), nm="NM" in self.info_order, phase=bool(cfg.phase), symbolic=bool(cfg.symbolic),
                    minsvlen=int(cfg.minsvlen), genotype_format=self.genotype_format,
                    genotype_none=format_genotype(self.default_genotype, cfg.phase))
        order = np.ascontiguousarray(order, np.int64)
        extra = ()
        ref = self.reference_handle
        if ref is not None and not cfg.symbolic and len(order):      # (--symbolic fetches nothing, vcf.py:318-324)
            # what `_resolve_sequences` fetches per call, as two batches on the device-resident reference: the deleted bases of every
            # deletion up to max_del_seq_len, and the base at max(0, pos - 1) of every record
            from .soa import SVTYPES
            calls = res.calls[order]
            pos, svlen = calls["pos"].astype(np.int64), calls["svlen"].astype(np.int64)
            is_del = (calls["svtype"] == SVTYPES.index("DEL")) & (np.abs(svlen) <= int(cfg.max_del_seq_len))
            del_idx = np.full(len(order), -1, np.int64)
            del_idx[is_del] = np.arange(int(is_del.sum()))
            dpool, doff, dst, dn = ref.fetch_many(ti.contig, (pos - 1)[is_del], (pos - svlen)[is_del])
            start = np.maximum(0, pos - 1)
            bpool, boff, bst, _ = ref.fetch_many(ti.contig, start, start + 1)
            extra = ((del_idx, dpool, doff, dst, dn, bpool, boff, bst, float(cfg.max_unknown_pct)),)
        text, n = _fast().vcf_records(np.ascontiguousarray(res.calls), order,
                                      np.ascontiguousarray(res.rnames, np.uint32), np.ascontiguousarray(res.alt_pool, np.uint8),
                                      ti.qnames, ti.ps_names, ti.contig, int(ti.task_id), ti.contig_names, list(_filters()), opts, *extra)
        self.handle.write(text.decode("utf-8"))
        self.call_count += n
        return n

    # ---- force calling: targets in, the same lines with this sample's genotype out (vcf.py:352-481)
    @staticmethod
    def _parse_target(line):
        """One non-header record of a target VCF as `read_svs_iter` reads it (vcf.py:352-430), in the reference's order of evaluation
        (so that a malformed line fails with the same exception): (chrom, pos0, ref, alt, qual, filter, info, svtype, svlen, end, bnd)
        with `bnd` = (mate_contig, mate_ref_start, is_first, is_reverse) or None."""
        chrom, pos, _, ref, alt, qual, flt, info_text = line.split("\t")[:8]
        info = {}
        for item in info_text.split(";"):
            if "=" in item:
                key, value = item.split("=")
            else:
                key, value = item, True
            info[key] = value
        pos0 = int(pos) - 1
        qual = int(qual) if qual != "." else None
        if len(alt) > len(ref):
            svtype, svlen, end = "INS", len(alt), pos0
        else:
            svtype, svlen = "DEL", -len(ref)
            end = pos0 + svlen
        if "SVTYPE" in info:
            svtype = "BND" if info["SVTYPE"] == "TRA" else info["SVTYPE"]
        if "SVLEN" in info:
            svlen = int(info["SVLEN"])
        if "END" in info:
            end = int(info["END"])
        bnd = None
        if svtype == "BND":
            parts = alt.replace("]", "[").split("[")
            if len(parts) <= 2:
                raise ValueError("BND ALT not formatted according to VCF 4.2 specifications")
            mate_contig, mate_pos = parts[1].split(":")
            bnd = (mate_contig, int(mate_pos), alt[0] == "N", "]" in alt)
        return chrom, pos0, ref, alt, qual, flt, info, svtype, svlen, end, bnd

    @classmethod
    def _read_target_line(cls, line_index, line):
        """One line of a target VCF (text or bytes): (its stripped text, None) for a header line, (its stripped text, `_parse_target` of
        the line) for a record.  A malformed line raises as the reference's reader does."""
        try:
            if isinstance(line, bytes):
                line = line.decode("utf-8")
            text = line.strip()
            if text == "":
                raise IndexError("string index out of range")     # the reference indexes the empty string here
            if text[0] == "#":
                return text, None
            return text, cls._parse_target(line)
        except Exception as e:
            raise ValueError(f"Error parsing input VCF: Line {line_index}: {e}") from e     # the reference exits here

    def _target_lines(self):
        """(1-based line number, the line, its stripped text) of every record of `self.handle` (text or bytes lines); header lines go
        to `self.header_str`.  A malformed line raises as the reference's reader does; the caller parses inside the same guard."""
        self.header_str = ""
        for line_index, line in enumerate(self.handle, 1):
            text, parsed = self._read_target_line(line_index, line)
            if parsed is None:
                self.header_str += text + "\n"
                continue
            yield line_index, text, parsed

    def read_svs_iter(self):
        """Target SVs of `--genotype-vcf`: one `SVCall` per record of `self.handle` (text or bytes lines); header lines
        are collected in `self.header_str`.  Type and length come from REF / ALT unless INFO gives SVTYPE (`TRA` = BND),
        SVLEN, END; a BND's mate is parsed from its ALT.  `call.id` is the 1-based line number, like the reference."""
        from . import sv
        for line_index, text, (chrom, pos0, ref, alt, qual, flt, info, svtype, svlen, end, bnd) in self._target_lines():
            call = sv.SVCall(contig=chrom, pos=pos0, id=line_index, ref=ref, alt=alt, qual=qual,
                             filter=flt, info=info, svtype=svtype, svlen=svlen, end=end, rnames=None, qc=True, postprocess=None,
                             genotypes=None, precise=None, support=0, fwd=0, rev=0, nm=-1)
            if bnd is not None:
                call.bnd_info = sv.SVCallBNDInfo(mate_contig=bnd[0], mate_ref_start=bnd[1], is_first=bnd[2], is_reverse=bnd[3])
            call.raw_vcf_line, call.raw_vcf_line_index = text, line_index
            yield call

    def read_target_table(self) -> dict:
        """The records `read_svs_iter` reads, as one column table per contig (contigs in order of first appearance, records in input
        order) and without an `SVCall`: {contig: dict(line_index, svtype, pos, svlen, end, mate_contig, mate_ref_start, bnd_is_first,
        bnd_is_reverse, cov, lines, mate_names)}.  `svtype`: the SNF_* code of a type in `sv.TYPES`, else -1 (`svtype_names` keeps the
        strings); `mate_contig`: index into the contig's `mate_names`, -1 without a mate; `cov`: [n, 5] zeros - the coverage fields a
        fresh `SVCall` has (sv.py:117-121); `lines`: the stripped text of every record (`raw_vcf_line`).  Same rules, same 1-based line
        numbers and the same ValueError for a malformed line as `read_svs_iter`."""
        import numpy as np

        from . import sv
        code = {n: k for k, n in enumerate(sv.TYPES)}
        rows = {}
        for line_index, text, (chrom, pos0, _, _, _, _, _, svtype, svlen, end, bnd) in self._target_lines():
            t = rows.get(chrom)
            if t is None:
                t = rows[chrom] = dict(line_index=[], svtype=[], svtype_names=[], pos=[], svlen=[], end=[], mate_contig=[], mate_ref_start=[],
                                       bnd_is_first=[], bnd_is_reverse=[], lines=[], mate_names=[], _mates={})
            t["line_index"].append(line_index); t["svtype"].append(code.get(svtype, -1)); t["svtype_names"].append(svtype)
            t["pos"].append(pos0); t["svlen"].append(svlen); t["end"].append(end); t["lines"].append(text)
            if bnd is None:
                t["mate_contig"].append(-1); t["mate_ref_start"].append(0); t["bnd_is_first"].append(0); t["bnd_is_reverse"].append(0)
            else:
                k = t["_mates"].get(bnd[0])
                if k is None:
                    k = t["_mates"][bnd[0]] = len(t["mate_names"])
                    t["mate_names"].append(bnd[0])
                t["mate_contig"].append(k); t["mate_ref_start"].append(bnd[1]); t["bnd_is_first"].append(int(bnd[2])); t["bnd_is_reverse"].append(int(bnd[3]))
        for t in rows.values():
            del t["_mates"]
            for k in ("line_index", "pos", "svlen", "end", "mate_ref_start"):
                t[k] = np.asarray(t[k], np.int64)
            t["svtype"], t["mate_contig"] = np.asarray(t["svtype"], np.int32), np.asarray(t["mate_contig"], np.int32)
            t["bnd_is_first"], t["bnd_is_reverse"] = np.asarray(t["bnd_is_first"], np.uint8), np.asarray(t["bnd_is_reverse"], np.uint8)
            t["cov"] = np.zeros((len(t["lines"]), 5), np.int32)
        return rows

    def read_target_table_device(self, source, device: int = 0, max_grid: int = 0, run_bytes: int = 256 << 20) -> dict:
        """`read_target_table` of `io.BytesIO(<the inflated bytes of source>)` with the text in HBM (csrc/snf_vcftext.h): `source` is a
        path or the file's bytes - plain, bgzip (inflated on the device) or gzip.  The same keys, dtypes, order and `header_str`; `lines`
        is a `DeviceTargetLines` (it answers `len()` and `[i]` and fetches the text when asked).  The kernel fills the columns of every
        line it is certain about; the others (`self.host_lines`, 1-based; `self.n_host_lines` of them) go through `_read_target_line` in
        file order: the first that raises is the file's first error, the others patch their row or join the header.  The host's part
        is over runs of equal CHROM (contigs in order of first appearance; a contig that reappears appends), over the BND rows (mate
        names per contig in order of first appearance) and over the host lines - not over the lines.  `self.target_timing`: the kernels' ms."""
        import os

        import numpy as np

        from . import abi, lib as L, sv
        if isinstance(source, (bytes, bytearray, memoryview)):
            data = bytes(source)
        elif isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as f:
                data = f.read()
        else:
            raise TypeError("read_target_table_device takes a path or the file's bytes, not an open handle "
                            f"({type(source).__name__}): the text goes to the device as one block")
        text = L.VcfText(data, device, run_bytes, max_grid)
        try:
            return self._device_table(text, text.parse(), np, abi, sv)
        except Exception:
            text.close()
            raise

    def _device_table(self, text, tab, np, abi, sv) -> dict:
        self.header_str = ""
        self.target_timing = dict(text.timing)
        cls, start = tab["cls"], tab["start"]
        raw_len = np.append(start[1:], text.text_len) - start if len(tab) else np.zeros(0, np.int64)
        host_ids = np.flatnonzero(cls == abi.VT_HOST)
        self.n_host_lines, self.host_lines = int(len(host_ids)), (host_ids + 1).tolist()
        host_rows, headers = {}, {}
        if len(host_ids):
            for k, raw in zip(host_ids.tolist(), text.strings(start[host_ids], raw_len[host_ids])):
                stripped, parsed = self._read_target_line(k + 1, raw)
                if parsed is None:
                    headers[k] = stripped
                else:
                    host_rows[k] = (stripped, parsed)
        hdr_ids = np.flatnonzero(cls == abi.VT_HEADER)
        for k, raw in zip(hdr_ids.tolist(), text.strings(start[hdr_ids], tab["send"][hdr_ids])):
            headers[k] = raw.decode("utf-8")
        self.header_str = "".join(headers[k] + "\n" for k in sorted(headers))
        is_row = cls == abi.VT_RECORD
        if host_rows:
            is_row = is_row.copy()
            is_row[list(host_rows)] = True
        rows = np.flatnonzero(is_row)
        n = int(len(rows))
        if n == 0:
            text.close()
            return {}
        r = tab[rows]
        on_host = r["cls"] != abi.VT_RECORD
        col = dict(line_index=(rows + 1).astype(np.int64), svtype=r["svtype"].astype(np.int32), pos=r["pos"].astype(np.int64),
                   svlen=r["svlen"].astype(np.int64), end=r["end"].astype(np.int64), mate_ref_start=r["mate_pos"].astype(np.int64),
                   bnd_is_first=(r["flags"] & abi.VT_BND_FIRST).astype(np.uint8), bnd_is_reverse=((r["flags"] & abi.VT_BND_REVERSE) >> 1).astype(np.uint8))
        type_names = np.array(sv.TYPES + [None], object)[col["svtype"]]
        mate = np.full(n, None, object)
        chrom = {}                                      # row -> CHROM, for the rows that open a run
        new_run = (r["flags"] & abi.VT_NEW_CHROM) != 0
        new_run[0] = True
        # the spans the table needs as strings, in one fetch: names of other types, mates, the CHROM of every run
        other = np.flatnonzero(~on_host & (col["svtype"] < 0))
        bnd = np.flatnonzero(~on_host & (col["svtype"] == sv.TYPES.index("BND")))
        code = {name: k for k, name in enumerate(sv.TYPES)}
        host_text = {}
        for i in np.flatnonzero(on_host).tolist():      # the rows the host parsed: every column from `_parse_target`
            stripped, (c, pos0, _, _, _, _, _, svtype, svlen, end, b) = host_rows[int(rows[i])]
            host_text[int(rows[i])] = (stripped, "\t".join(stripped.split("\t")[:8]).encode("utf-8"))      # (and what the rewrite keeps of it)
            col["svtype"][i], col["pos"][i], col["svlen"][i], col["end"][i] = code.get(svtype, -1), pos0, svlen, end
            type_names[i] = svtype
            col["mate_ref_start"][i], col["bnd_is_first"][i], col["bnd_is_reverse"][i] = (0, 0, 0) if b is None else (b[1], int(b[2]), int(b[3]))
            if b is not None:
                mate[i] = b[0]
            chrom[i] = c
            new_run[i] = True
            if i + 1 < n:
                new_run[i + 1] = True
        opens = np.flatnonzero(new_run & ~on_host)
        want = np.concatenate([other, bnd, opens])
        span_off = np.concatenate([r["start"][other] + r["span_a"][other], r["start"][bnd] + r["span_a"][bnd], r["start"][opens]])
        span_len = np.concatenate([r["span_len"][other], r["span_len"][bnd], r["chrom_end"][opens]]).astype(np.int64)
        got = [b.decode("utf-8") for b in text.strings(span_off, span_len)] if len(want) else []
        type_names[other] = got[:len(other)]
        mate[bnd] = got[len(other):len(other) + len(bnd)]
        for i, c in zip(opens.tolist(), got[len(other) + len(bnd):]):
            chrom[i] = c
        # runs of equal CHROM -> contigs
        run_at = np.flatnonzero(new_run)
        run_end = np.append(run_at[1:], n)
        parts = {}
        for a, b in zip(run_at.tolist(), run_end.tolist()):
            parts.setdefault(chrom[a], []).append((a, b))
        out = {}
        for c, spans in parts.items():
            idx = np.arange(spans[0][0], spans[0][1]) if len(spans) == 1 else np.concatenate([np.arange(a, b) for a, b in spans])
            names, seen = [], {}
            mate_contig = np.full(len(idx), -1, np.int32)
            m = mate[idx]
            for j in np.flatnonzero(m != None).tolist():  # noqa: E711 - elementwise
                k = seen.get(m[j])
                if k is None:
                    k = seen[m[j]] = len(names)
                    names.append(m[j])
                mate_contig[j] = k
            out[c] = dict(line_index=col["line_index"][idx], svtype=col["svtype"][idx], svtype_names=type_names[idx].tolist(), pos=col["pos"][idx],
                          svlen=col["svlen"][idx], end=col["end"][idx], mate_contig=mate_contig, mate_ref_start=col["mate_ref_start"][idx],
                          bnd_is_first=col["bnd_is_first"][idx], bnd_is_reverse=col["bnd_is_reverse"][idx],
                          lines=DeviceTargetLines(text, rows[idx], r["start"][idx], r["send"][idx].astype(np.int64), host_text), mate_names=names,
                          cov=np.zeros((len(idx), 5), np.int32))
        return out

    @staticmethod
    def select_targets(table: dict, keep) -> dict:
        """The rows `keep` (boolean mask or indices) of one contig's target table, order kept."""
        import numpy as np
        idx = np.flatnonzero(keep) if np.asarray(keep).dtype == bool else np.asarray(keep, np.int64)
        out = {}
        for k, v in table.items():
            if k == "mate_names":
                out[k] = v
            elif isinstance(v, list):
                out[k] = [v[i] for i in idx.tolist()]
            else:
                out[k] = v[idx]
        return out

    def rewrite_header_genotype(self, orig_header: str):
        lines = orig_header.split("\n")
        cfg = self.config
        lines[1:1] = [f"##genotypeSource={cfg.version}_{cfg.build}", f'##genotypeCommand="{cfg.command}"',
                      f'##genotypeFileDate="{cfg.start_date}"']
        for ident, number, typ, desc in _FORMAT[:4]:          # GT, GQ, DR, DV: added if the input does not declare them
            if not any(f"##FORMAT=<ID={ident}," in ln for ln in lines):
                lines.insert(len(lines) - 2, f'##FORMAT=<ID={ident},Number={number},Type={typ},Description="{desc}">')
        self.write_raw("\n".join(lines), endl="")

    def rewrite_genotype(self, svcall):
        """The target's own line (first eight columns) with FORMAT and this sample's genotype: the matched candidate's
        if there is one and it was genotyped, else the reference-allele genotype from the coverage (parallel.py:355-366)."""
        match = svcall.genotype_match_sv
        gt = match.genotypes[0] if (match is not None and len(match.genotypes) > 0) else svcall.genotypes[0]
        cols = svcall.raw_vcf_line.split("\t")[:8] + [self.config.genotype_format, format_genotype(gt, self.config.phase)]
        self.write_raw("\t".join(cols))

    def rewrite_genotype_records(self, lines, genotypes) -> int:
        """`rewrite_genotype` for the targets of one contig from their raw lines and genotype tuples (`GenotypeTask.genotype_tuples`):
        the first eight columns + FORMAT + the sample column, assembled here and written once.  Returns the number of lines."""
        fmt, phase = self.config.genotype_format, self.config.phase
        cache = {}
        out = []
        for text, gt in zip(lines, genotypes):
            col = cache.get(gt)
            if col is None:
                col = cache[gt] = fmt + "\t" + format_genotype(gt, phase)
            out.append("\t".join(text.split("\t")[:8]))
            out.append("\t")
            out.append(col)
            out.append("\n")
        if out:
            self.handle.write("".join(out))
        return len(out) // 4

    def rewrite_genotype_device(self, lines_obj, rows, gt, tuples=None, max_grid: int = None, distinct=None) -> int:
        """`rewrite_genotype_records(lines, genotypes)` for the `DeviceTargetLines` of a contig, assembled where the text lies: `rows`
        selects and orders the lines (indices into `lines_obj`; None: all of them), `gt` is the [n, 8] column of `execute_records` with
        `tuples` the function that turns such rows into genotype tuples (`lambda g: task.genotype_tuples({"gt": g})`), or the list of
        tuples itself; `distinct=(tuples of the distinct rows, inverse)` hands over what the caller already worked out (`_distinct_rows`; `gt` is
        then not read).  The distinct genotypes are formatted once by `format_genotype` and go up as a suffix table; vt_size / vt_copy
        put the first eight columns of every line in front of its suffix, and one block comes back.  Rows the host parsed are assembled
        here and spliced in.  The same text, byte for byte.  Returns the number of lines."""
        import io

        import numpy as np
        if rows is not None:
            lines_obj = lines_obj[np.asarray(rows, np.int64)]
        n = len(lines_obj)
        fmt, phase = self.config.genotype_format, self.config.phase
        if distinct is not None:
            distinct, sid = list(distinct[0]), np.asarray(distinct[1], np.int32).reshape(-1)
            if len(sid) != n or (n and not (0 <= int(sid.min()) and int(sid.max()) < len(distinct))):
                raise ValueError(f"rewrite_genotype_device: {n} lines, {len(sid)} genotypes over {len(distinct)} distinct ones")
            if n == 0:
                return 0
        elif tuples is not None:
            gt = np.asarray(gt).reshape(-1, 8)
            if len(gt) != n:
                raise ValueError(f"rewrite_genotype_device: {n} lines, {len(gt)} genotypes")
            if n == 0:
                return 0
            uniq, inverse = _distinct_rows(gt)
            distinct, sid = tuples(uniq), np.asarray(inverse, np.int32).reshape(-1)
        else:
            gt = list(gt)
            if len(gt) != n:
                raise ValueError(f"rewrite_genotype_device: {n} lines, {len(gt)} genotypes")
            if n == 0:
                return 0
            seen = {}
            sid = np.asarray([seen.setdefault(g, len(seen)) for g in gt], np.int32)
            distinct = list(seen)
        suffixes = [("\t" + fmt + "\t" + format_genotype(g, phase) + "\n").encode("utf-8") for g in distinct]
        line = lines_obj.line.copy()
        on_host = np.isin(line, lines_obj.host_ids) if len(lines_obj.host_ids) else np.zeros(n, bool)
        line[on_host] = -1
        text = lines_obj.text
        if max_grid is not None:
            keep, text.max_grid = text.max_grid, int(max_grid)
        try:
            raw, off = text.rewrite(line, sid, suffixes)
        finally:
            if max_grid is not None:
                text.max_grid = keep
        self.rewrite_kernel_ms = text.last_ms
        if on_host.any():
            pieces, at = [], 0
            for i in np.flatnonzero(on_host).tolist():
                pieces.append(raw[at:int(off[i])])
                at = int(off[i])
                pieces.append(lines_obj.host_text[int(lines_obj.line[i])][1] + suffixes[int(sid[i])])
            pieces.append(raw[at:])
            raw = b"".join(pieces)
        h = self.handle
        if isinstance(h, io.TextIOBase):
            under = getattr(h, "buffer", None)      # a text file over a binary one: the bytes go as they are
            if under is not None and getattr(h, "encoding", "").lower().replace("-", "") == "utf8":      # (as write_merged does)
                h.flush()
                under.write(raw)
            else:
                h.write(raw.decode("utf-8"))
        else:
            h.write(raw)                            # a binary handle (bgzfout.BgzfWriter / VcfGzWriter take bytes)
        return n


def _distinct_rows(a):
    """`np.unique(a, axis=0, return_inverse=True)` of an integer table up to the order of the distinct rows: (rows, inverse) with
    `rows[inverse] == a`.  The row-wise unique sorts records of the row's width (measured on 200 000 x 8: half the time of the whole
    device text path); here every column is ranked on its own and the ranks are folded into one integer per row - exact, no hashing -
    as long as the product of the columns' cardinalities fits 62 bits, which genotype rows always do; else the row-wise unique."""
    import numpy as np
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.dtype.kind not in "iu" or len(a) == 0:
        return np.unique(a, axis=0, return_inverse=True)
    key, radix = np.zeros(len(a), np.int64), 1
    for j in range(a.shape[1]):
        vals, code = np.unique(a[:, j], return_inverse=True)
        if radix * len(vals) >= 1 << 62:
            return np.unique(a, axis=0, return_inverse=True)
        key += code.reshape(-1).astype(np.int64) * radix
        radix *= len(vals)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    return a[first], inverse.reshape(-1)


class DeviceTargetLines:
    """The `lines` column of a target table whose text lives in HBM (`VCF.read_target_table_device`): the handle, the 0-based line of
    every row and where its stripped text lies.  `len()`, `[i]` (the stripped text, as `read_target_table` keeps it), `[indices]` /
    `[mask]` / `[slice]` (the same object over those rows: what `VCF.select_targets` asks for) and iteration; the text of the rows is
    fetched when one of them is asked for, once.  Rows the host parsed carry their text (`host_text`, by line: the stripped text and its
    first eight columns; one dict for the whole file, so a row is looked up by `np.isin` against `host_ids`, never by a loop over rows).
    `close()` frees the text in HBM - for every table of the file, they share the handle."""

    def __init__(self, text, line, start, send, host_text, host_ids=None):
        import numpy as np
        self.text, self.line, self.start, self.send, self.host_text = text, line, start, send, host_text
        self.host_ids = np.fromiter(host_text, np.int64, len(host_text)) if host_ids is None else host_ids
        self._cache = None

    def close(self):
        self.text.close()

    def __len__(self):
        return int(len(self.line))

    def _all(self):
        if self._cache is None:
            got = [b.decode("utf-8") for b in self.text.strings(self.start, self.send)]
            if len(self.host_ids):
                import numpy as np
                for i in np.flatnonzero(np.isin(self.line, self.host_ids)).tolist():
                    got[i] = self.host_text[int(self.line[i])][0]
            self._cache = got
        return self._cache

    def __getitem__(self, i):
        import numpy as np
        if isinstance(i, (int, np.integer)):
            return self._all()[int(i)]
        if not isinstance(i, slice):
            i = np.asarray(i)
            i = np.flatnonzero(i) if i.dtype == bool else i.astype(np.int64)
        return DeviceTargetLines(self.text, self.line[i], self.start[i], self.send[i], self.host_text, self.host_ids)

    def __iter__(self):
        return iter(self._all())

