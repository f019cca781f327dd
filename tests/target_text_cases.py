"""Builders for tests/test_target_text.py: target VCF texts whose line starts, tabs, INFO keys and line lengths sit on the borders of the
device kernels' work units (sniffles_amd/csrc/snf_vcftext.h), the directed table of the grammar, and the lines the device must leave to
the host.  The unit sizes are read from the source, as tests/fasta_cases.py does: a literal that is no longer found is an error.

vt_parse walks a line in steps of VT_STEP bytes from the aligned 16-byte word that holds the line's first byte: a lane border is every
multiple of VT_VEC behind that word, a step border every multiple of VT_STEP.  `aligned` puts a record at a chosen offset modulo VT_VEC,
so that an offset inside the line is an offset inside the walk."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit_sizes():
    with open(os.path.join(ROOT, "sniffles_amd", "csrc", "snf_vcftext.h")) as f:
        src = f.read()
    out = {}
    for name in ("VT_VEC", "VT_WG", "VT_STEP", "VT_CHUNK", "VT_CHROM_WG", "VT_MAX_DIGITS"):
        m = re.findall(rf"^#define {name} (\d+)\b", src, re.M)
        if len(m) != 1:
            raise AssertionError(f"target_text_cases: expected exactly one #define {name} in snf_vcftext.h, found {len(m)}")
        out[name] = int(m[0])
    assert out["VT_STEP"] == 64 * out["VT_VEC"] and out["VT_CHUNK"] == out["VT_WG"] * out["VT_VEC"]
    return out


S = unit_sizes()
VEC, STEP, CHUNK, CHROM_WG, DIGITS = S["VT_VEC"], S["VT_STEP"], S["VT_CHUNK"], S["VT_CHROM_WG"], S["VT_MAX_DIGITS"]

HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
GOOD_INFO = "SVTYPE=DEL;SVLEN=-50;END=150"


def rec(chrom="chr1", pos="100", ident="id", ref="N", alt="<DEL>", qual="60", flt="PASS", info=GOOD_INFO, tail="GT\t0/1", nl="\n") -> bytes:
    """One record line; `tail` None: eight columns."""
    cols = [chrom, str(pos), ident, ref, alt, str(qual), flt, info] + ([] if tail is None else [tail])
    return ("\t".join(cols) + nl).encode("latin-1")


def pad_to(text: bytes, offset: int) -> bytes:
    """`text` followed by header lines, `offset` bytes in all (the next line starts there)."""
    need = offset - len(text)
    if need == 0:
        return text
    if need < 3:                       # no room for "##\n": lengthen the line in front instead
        assert text.endswith(b"\n") and text.rstrip(b"\n").split(b"\n")[-1].startswith(b"#"), "pad_to needs a header line in front"
        return text[:-1] + b"x" * need + b"\n"
    return text + b"##" + b"p" * (need - 3) + b"\n"


def aligned(lines, mod=0, start=HEAD) -> bytes:
    """The lines one behind the other, each at an offset that is `mod` modulo VT_VEC (header lines fill up)."""
    text = start
    for ln in lines:
        at = len(text) + 3
        at += (mod - at) % VEC
        text = pad_to(text, at) + ln
    return text


def line_start_texts():
    """A record whose first byte - and so the '\\n' in front of it - lies at -1 / 0 / +1 of a word and of a chunk."""
    out = {}
    for name, b in (("word", VEC * 6), ("chunk", CHUNK), ("chunk2", 2 * CHUNK)):
        for d in (-1, 0, 1):
            out[f"line_at_{name}{d:+d}"] = pad_to(HEAD, b + d) + rec() + rec(chrom="chr2", info="SVLEN=7")
            out[f"last_line_at_{name}{d:+d}_no_newline"] = pad_to(HEAD, b + d) + rec(tail=None, nl="")
    # a '\n' as the last byte of a chunk with nothing behind it: no line starts at the text's end
    out["text_ends_at_chunk"] = pad_to(HEAD, CHUNK - len(rec())) + rec()
    assert len(out["text_ends_at_chunk"]) == CHUNK
    return out


PREFIX = "chr1\t100\t"          # what stands in front of ID


def info_at(offset: int, info: str, tail="GT\t0/1") -> bytes:
    """A record whose INFO column starts `offset` bytes into the line (ID takes the room)."""
    fixed = len(PREFIX) + len("\tN\t<DEL>\t60\tPASS\t")
    assert offset - fixed >= 1, offset
    return rec(ident="i" * (offset - fixed), info=info, tail=tail)


def key_split_lines():
    """Every byte of `SVTYPE=`, `SVLEN=`, `END=` - and the ';' in front and the value behind - on either side of a lane border and of the
    step border; the same for a ';' and an '=' of other items."""
    out = []
    for border in (VEC * 5, STEP, 2 * STEP):
        for key, value in (("SVTYPE=", "INV"), ("SVLEN=", "-123"), ("END=", "4567"), ("SVTYPE=", "TRA"), ("SVTYPE=", "OTHER")):
            for j in range(-1, len(key) + len(value) + 2):
                # the key's first byte at border - j: INFO = "AA=1;" + key ... so that the ';' in front is walked too
                lead = "AA=1;"
                alt = "N[chr9:5[" if value == "TRA" else "<DEL>"
                ln = info_at(border - j - len(lead) - (len(alt) - 5), lead + key + value + ";ZZ=2")
                if alt != "<DEL>":
                    ln = ln.replace(b"<DEL>", alt.encode())
                assert ln.index(key.encode() + value.encode()) == border - j
                out.append(ln)
        for d in (-1, 0, 1):            # the eighth tab, and the seventh, at the border
            out.append(info_at(border + d - len(GOOD_INFO), GOOD_INFO))
            out.append(info_at(border + d, GOOD_INFO))
            out.append(info_at(border + d, GOOD_INFO, tail=None))
            out.append(info_at(border + d - 4, "A=1;B;;SVLEN=9"))      # ';' and '=' around it
    return out


def length_lines():
    out = []
    for n in (STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1):
        for tail in ("GT\t0/1", None):
            base = rec(ident="", tail=tail)
            out.append(rec(ident="L" * (n - len(base)), tail=tail))
            assert len(out[-1]) == n
    out.append(rec(ref="N", alt="N" + "ACGT" * 17500, info="SUPPORT=3", tail="GT:GQ\t1/1:9"))       # a long ALT: INS by length, 70 001 bases
    out.append(rec(ref="N" + "ACGT" * 700, alt="N", info="SUPPORT=3;RNAMES=" + ",".join("read%d" % k for k in range(900))))
    long_info = "PRECISE;RNAMES=" + ",".join("r%05d" % k for k in range(600)) + ";SVTYPE=DUP;SVLEN=88;END=99"      # the keys in the last step
    assert len(long_info) > 3 * STEP
    out.append(rec(info=long_info))
    out.append(rec(info="SVTYPE=INS;SVLEN=1;END=2;RNAMES=" + "q" * (2 * STEP) + ";SVLEN=5;STRAND=+-"))      # ... and one again, steps later: the last wins
    out.append(rec(alt="N" + "A" * (STEP + 40) + "[chr7:123[", info="SVTYPE=BND"))                # brackets behind the first step of ALT
    out.append(rec(alt="]" + "c" * (STEP + 3) + ":77]N", info="SVTYPE=BND"))                      # a mate name longer than a step
    return out


def many_lines(n: int, per: int = 3) -> bytes:
    """n record lines, CHROM changing every `per` lines."""
    return HEAD + b"".join(rec(chrom="chr%d" % (k // per), pos=100 + k, info="SVLEN=%d" % (k + 50)) for k in range(n))


def chrom_run_text() -> bytes:
    """Runs of CHROM that begin at -1 / 0 / +1 of vt_chrom's workgroup (lines, header included), a contig that comes back, and names that
    differ in their last byte only or in their length only."""
    lines = HEAD.count(b"\n")
    out = [HEAD]
    for k in range(3 * CHROM_WG):
        block, m = divmod(lines + k, CHROM_WG)      # (0-based line, header included)
        if block == 0:
            name = "chrA"
        elif block == 1:
            name = "b2x_" if m == CHROM_WG - 1 else "b1x"                                   # one line in front of the border: the length only
        elif block == 2:
            name = "b2x" if m == 0 else "chrA" if m == CHROM_WG - 1 else "b2y"              # at the border; one behind it: the last byte only
        else:
            name = "b3x"
        out.append(rec(chrom=name, pos=1000 + k, info="SVLEN=60"))
    return b"".join(out)


def directed_lines():
    """[(what, line)]: the grammar line by line.  The reference parser alone reads every one of them (no fallback is needed: the test
    asserts that none went to the host)."""
    big = "9" * DIGITS
    L = [
        # defaults and overrides
        ("ins_by_length", rec(ref="N", alt="NACGT", info="X=1")),
        ("del_by_length", rec(ref="NACGT", alt="N", info="X=1")),
        ("equal_lengths", rec(ref="AC", alt="GT", info="X=1")),
        ("svtype_alone", rec(ref="N", alt="NAAAA", info="SVTYPE=DUP")),
        ("svlen_alone", rec(info="SVLEN=-77")),
        ("end_alone", rec(info="END=999")),
        ("all_three", rec(info="END=5;SVTYPE=INV;SVLEN=12")),
        ("duplicate_keys", rec(info="SVTYPE=INS;SVLEN=1;END=2;SVTYPE=DEL;SVLEN=-3;END=4;SVLEN=-5")),
        ("duplicate_bad_then_good", rec(info="SVLEN=fifty;END=1.5;SVLEN=50;END=15")),
        # types
        ("tra", rec(alt="N[chr2:500[", info="SVTYPE=TRA")),
        ("unknown_type", rec(info="SVTYPE=CNV;SVLEN=10")),
        ("unknown_type_long", rec(info="SVTYPE=" + "Q" * 40)),
        ("type_lower_case", rec(info="SVTYPE=del")),
        ("type_empty", rec(info="SVTYPE=;SVLEN=3")),
        ("type_tra_prefix", rec(info="SVTYPE=TRAX")),
        # flags and prefixes
        ("flags_and_empty_items", rec(info="PRECISE;;SVLEN=8;;IMPRECISE;")),
        ("empty_info", rec(info="")),
        ("only_semicolons", rec(info=";;;")),
        ("prefix_keys", rec(info="SVLENX=1;XEND=2;CIEND=3;END2=4;XSVTYPE=INS;SVTYPES=INS;ENDX;SVLENGTH")),
        ("prefix_then_real", rec(info="CIEND=3;END=40;XSVLEN=1;SVLEN=-6")),
        ("key_as_value", rec(info="A=SVLEN;B=END;SVTYPE=END")),
        # extreme values
        ("negative", rec(pos="-5", info="SVLEN=-9;END=-3")),
        ("eighteen_digits", rec(pos=big, info="SVLEN=-" + big + ";END=" + big)),
        ("pos_zero", rec(pos="0", info="X")), ("pos_one", rec(pos="1", info="X")),
        ("leading_zeros", rec(pos="007", qual="000", info="SVLEN=-000")),
        ("qual_dot", rec(qual=".")), ("qual_negative", rec(qual="-1")),
        # column counts
        ("eight_columns", rec(tail=None)),
        ("eight_columns_crlf", rec(tail=None, nl="\r\n")),
        ("eight_columns_end_last", rec(info="SVTYPE=DEL;END=321", tail=None)),
        ("eight_columns_svlen_last_crlf", rec(info="SVLEN=-44", tail=None, nl="\r\n")),
        ("eight_columns_svtype_last", rec(info="SVLEN=4;SVTYPE=INS", tail=None)),          # the type is "INS\n": another name
        ("eight_columns_flag_last", rec(info="SVLEN=4;SVLEN", tail=None)),                 # the flag is "SVLEN\n": ignored
        ("nine_columns_crlf", rec(nl="\r\n")),
        ("nine_columns_trailing_blanks", rec(tail="GT\t0/1  \t ")),
        ("empty_columns_behind_info", rec(tail="\t")),
        ("two_hundred_columns", rec(tail="GT\t" + "\t".join("0/%d" % (k % 2) for k in range(191)))),
        ("chrom_with_a_blank", rec(chrom="chr 1")),
        # BND
        ("bnd_t[p[", rec(chrom="chr2", alt="N[chr5:100[", info="SVTYPE=BND")),
        ("bnd_t]p]", rec(chrom="chr2", alt="N]chr6:200]", info="SVTYPE=BND")),
        ("bnd_]p]t", rec(chrom="chr2", alt="]chr5:300]N", info="SVTYPE=BND")),
        ("bnd_[p[t", rec(chrom="chr2", alt="[chr7:400[N", info="SVTYPE=BND")),
        ("bnd_mixed_brackets", rec(chrom="chr2", alt="N[chr6:5]extra[", info="SVTYPE=BND")),
        ("bnd_colon_behind_the_second", rec(chrom="chr2", alt="N[chr6:5[:x:", info="SVTYPE=BND")),
        ("bnd_negative_mate", rec(chrom="chr2", alt="G[chr8:-4[", info="SVTYPE=BND;SVLEN=0")),
        ("bnd_empty_mate_name", rec(chrom="chr2", alt="N[:9[", info="SVTYPE=BND")),
        ("not_bnd_with_brackets", rec(chrom="chr2", alt="N[junk", info="SVTYPE=INS")),
    ]
    return L


def directed_text() -> bytes:
    """The directed lines; then a header line between records, mates reused and new per contig, a contig that reappears; the last line
    has eight columns and no '\\n'."""
    body = b"".join(ln for _, ln in directed_lines())
    more = (rec(chrom="chr3", alt="N[chr5:1[", info="SVTYPE=BND") + b"##a header line between records\n" +
            rec(chrom="chr3", alt="N[chr9:2[", info="SVTYPE=BND") + rec(chrom="chr3", alt="]chr5:3]N", info="SVTYPE=TRA") +
            rec(chrom="chr1", pos="5", info="SVLEN=1") + rec(chrom="chr2", alt="N[chr9:2[", info="SVTYPE=BND") +
            rec(chrom="chr3", info="END=77", tail=None, nl=""))
    return HEAD + body + more


# ---- lines the device leaves to the host: unusual but legal
def unusual_lines():
    """[(what, line)]: each is read by the reference parser without an error and must come out as the host reads it."""
    return [
        ("leading_space_before_hash", b" ##indented header\n"),
        ("pos_with_plus", rec(pos="+5")),
        ("pos_with_underscore", rec(pos="1_0")),
        ("svlen_with_a_blank", rec(info="SVLEN= 7")),
        ("flag_named_svlen", rec(info="SVLEN;END=9")),
        ("non_ascii_sample_column", rec(tail="GT\t0/1\t\xc3\xa9")),
        ("trailing_space_on_eight_columns", rec(info="SVLEN=5 ", tail=None)),
        ("nineteen_digits", rec(pos="1" + "0" * DIGITS)),
        ("non_ascii_header", b"##source=caf\xc3\xa9\n"),
        ("bnd_on_host", rec(alt="N[chr4:1_0[", info="SVTYPE=BND")),
        ("carriage_return_inside", rec(ident="a\rb")),
    ]
