"""The population SNF (`src/sniffles/snfp.py`): a merged population as a file of variants with their allele
frequencies, and the annotation of merged calls from it (`--combine-population`: `POPULATION_AF` / `POPULATION_SIZE`).

* `PopulationVariant.match` (snfp.py:91-107): does a call match a population variant?  It gates on position / length like the merge
  (`combine_match`, `combine_match_max`) and, for insertions, on `edlib.align(self.alt, svcall.alt)['editDistance']`.  `match_batch`
  serves given (variant, call) pairs - every alignment one entry of ONE `snf_edit_distance_batch` launch.
* `PopulationSNF` (snfp.py:118-192) is the container: same header, index and gzip-pickled blocks as a sample's `.snf`
  (`snf.SNFileBase`), the blocks hold `PopulationVariant` records instead of calls and the header carries a `population` entry.
  Files written here are read by the reference and the other way round.
* `PopulationSNF.get_population_AF_batch` answers `get_population_AF` (snfp.py:131-155) for ALL calls of a merge in one launch
  (`snf_population_match_batch`, include/sniffles_amd.h): the file's variant lists are laid out once as a CSR table
  (`PopulationSNF.table`), a call is one query against the list of its (contig, block, SV type), and the kernel orders the alignments
  so that most of them are never run.

The record below has the reference's fields, so objects unpickled from a reference-written population SNF work as they are (anything
with `pos`, `svlen`, `svtype`, `alt`).
"""
from __future__ import annotations

import math
import os
from dataclasses import asdict, dataclass
from typing import Optional

import numpy as np

from . import lib, snf, sv


@dataclass
class PopulationVariant:
    contig: str
    pos: int
    id: str
    alt: str
    svtype: str
    svlen: int
    end: int
    af: float
    genotyped_sample_count: int
    variant_sample_count: int

    @staticmethod
    def _calculate_frequency(genotypes: dict, ploidy: int = 2):
        """(population AF, genotyped samples, samples carrying the SV) from {sample id: genotype tuple} (snfp.py:40-64)."""
        total = variant = genotyped = carrying = 0
        for gt in genotypes.values():
            if gt[0] == '.':
                continue
            genotyped += 1
            n = gt[0] + gt[1]
            total += ploidy
            variant += n
            if n > 0:
                carrying += 1
        return variant / total, genotyped, carrying

    @classmethod
    def from_svcall(cls, svcall, config) -> Optional["PopulationVariant"]:
        """The population variant of a merged call, or None when too few samples are genotyped for it (snfp.py:65-89;
        `config` stands for the reference's `SnifflesConfig.GLOBAL`)."""
        af, genotyped, carrying = cls._calculate_frequency(svcall.genotypes, config.genotype_ploidy)
        if genotyped / len(config.snf_input_info) < config.dev_population_min_gt:
            return None
        return cls(contig=svcall.contig, pos=svcall.pos, id=svcall.id, alt=svcall.alt, svtype=svcall.svtype, svlen=svcall.svlen,
                   end=svcall.end, af=af, genotyped_sample_count=genotyped, variant_sample_count=carrying)

    def match(self, svcall, config, device: int = 0) -> Optional[int]:
        """The distance (smaller is better) or None when `svcall` is not this variant (snfp.py:91-107)."""
        return match_batch([(self, svcall)], config, device)[0]


snf.register_record_class("sniffles.snfp", "PopulationVariant", PopulationVariant)


@dataclass
class PopulationInfo:
    version: int
    name: str
    description: str
    size: int


def _gate(pv, svcall, config) -> Optional[int]:
    dist = abs(pv.pos - svcall.pos) + abs(abs(pv.svlen) - abs(svcall.svlen))
    minlen = float(min(abs(pv.svlen), abs(svcall.svlen)))
    if dist > config.combine_match * math.sqrt(minlen) or dist > config.combine_match_max:
        return None
    return dist


def match_batch(pairs, config, device: int = 0) -> list:
    """`pv.match(svcall)` for every (population variant, call) pair; the insertions' sequence comparisons of all pairs go to
    the GPU in one launch.  The reference rejects when `(svlen - d) / svlen <= combine_pctseq`, i.e. accepts iff
    d < (1 - pctseq) * svlen: that bound is the band of the alignment (distances beyond it need not be exact)."""
    out = [_gate(pv, sv, config) for pv, sv in pairs]
    limit = config.combine_pctseq
    todo = [k for k, (pv, sv) in enumerate(pairs) if out[k] is not None and pv.svtype == 'INS' and limit]
    if todo:
        seqs = [(pairs[k][0].alt.encode("latin-1"), pairs[k][1].alt.encode("latin-1")) for k in todo]
        # reject iff (svlen - d) / svlen <= limit  <=>  d >= svlen * (1 - limit): any distance >= that bound may come back as -1
        bounds = [max(0, int(math.ceil(abs(pairs[k][0].svlen) * (1.0 - limit))) + 1) for k in todo]
        d = lib.edit_distance_batch(seqs, device=device, max_dist=bounds)
        for k, dk in zip(todo, d.tolist()):
            pv = pairs[k][0]
            if dk < 0 or (pv.svlen - dk) / pv.svlen <= limit:
                out[k] = None
    return out


def _alt_bytes(alt: str) -> bytes:
    """The bytes the alignment compares: one per character (edlib compares the characters of the two strings)."""
    try:
        return alt.encode("latin-1")
    except UnicodeEncodeError:
        return alt.encode("utf-8")


class PopulationSNF(snf.SNFileBase):
    """A population SNF (snfp.py:118-192): reference interface - `open`, `read_header`, `store`, `get_population_AF` - plus the
    batch form the merge uses."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._blocks = {}
        self._table = None

    def _calculate_block_index(self, pos: int) -> int:
        return int(pos / self.config.snf_block_size) * self.config.snf_block_size

    # ---- writing
    def store(self, svcand) -> bool:
        """A merged call becomes a `PopulationVariant` of its block; False: dropped (`dev_population_min_gt`)."""
        variant = PopulationVariant.from_svcall(svcand, self.config)
        if variant is not None:
            super().store(variant)
        return variant is not None

    def _create_header(self, config, main_index: dict, snf_candidate_count: int) -> dict:
        d = super()._create_header(config, main_index, snf_candidate_count)
        d["population"] = asdict(PopulationInfo(version=1, name="Population", description="A sample population",
                                                size=len(config.snf_input_info)))
        return d

    def _calculate_contig_coverages(self, *args, **kwargs) -> dict:
        return {}                   # coverages are not used in population SNFs

    # ---- reading
    def read_header(self):
        super().read_header()
        try:
            self.header["population"] = PopulationInfo(**self.header["population"])
        except (KeyError, TypeError):
            pass                    # (the reference logs a warning and goes on)

    def table(self) -> dict:
        """The variant lists of the whole file as the CSR `lib.population_match_batch` takes, built once: one list per (contig,
        block key, SV type) in file order.  Like `get_population_AF` it looks a block up by the STRING `str(block start)` among
        the index's keys and reads only the FIRST part of a block (`get_all_blocks`, snf.py:231-239): later parts of a (contig,
        block) - a second task that wrote into it - are never searched.  Also: `keys` (sorted int64 key per list: contig number,
        block start, type number) with `key_list`, `contigs` / `types` (name -> number), and per variant `af` (rounded to 5
        places, as returned) and `size` (genotyped_sample_count)."""
        if self._table is not None:
            return self._table
        contigs, types = {}, {t: k for k, t in enumerate(sv.TYPES)}
        list_off, is_ins, keys = [0], [], []
        pos, svlen, af, size, alts = [], [], [], [], []
        for contig in self.index:
            ci = contigs.setdefault(contig, len(contigs))
            blocks = self._blocks.get(contig)
            if blocks is None:
                blocks = self._blocks[contig] = self.get_all_blocks(contig)
            for key, block in blocks.items():
                try:
                    start = int(key)
                except (TypeError, ValueError):
                    continue
                if str(start) != str(key) or not 0 <= start < (1 << 40):
                    continue            # no call's `str(int(...))` spells this key
                for svtype, variants in block.items():
                    if svtype == "_COVERAGE" or not isinstance(variants, list):
                        continue
                    ti = types.setdefault(svtype, len(types))
                    keys.append((ci << 44) | (start << 4) | ti)
                    is_ins.append(svtype == "INS")
                    for v in variants:
                        pos.append(v.pos); svlen.append(v.svlen); alts.append(_alt_bytes(v.alt))
                        af.append(round(v.af, 5)); size.append(v.genotyped_sample_count)
                    list_off.append(len(pos))
        if len(types) > 16:
            raise ValueError(f"'{self.filename}': more than 16 SV types in a population SNF")
        alt_off = np.zeros(len(alts) + 1, np.int64)
        if alts:
            np.cumsum(np.fromiter((len(a) for a in alts), np.int64, len(alts)), out=alt_off[1:])
        keys = np.asarray(keys, np.int64)
        order = np.argsort(keys, kind="stable")
        self._table = dict(list_off=np.asarray(list_off, np.int64), list_is_ins=np.asarray(is_ins, np.uint8),
                           v_pos=np.asarray(pos, np.int32), v_svlen=np.asarray(svlen, np.int32), v_alt_off=alt_off,
                           v_alt_pool=np.frombuffer(b"".join(alts) + b"\0", np.uint8), af=np.asarray(af, np.float64),
                           size=np.asarray(size, np.int64), keys=keys[order], key_list=order.astype(np.int32), contigs=contigs,
                           types=types)
        return self._table

    def _check_alignable(self, config) -> None:
        """An insertion with svlen <= 0 while the sequence gate is on: the reference divides by it (snfp.py:104)."""
        if not config.combine_pctseq:
            return
        t = self.table()
        ins = np.repeat(t["list_is_ins"], np.diff(t["list_off"])).astype(bool)
        bad = np.flatnonzero(ins & (t["v_svlen"] <= 0))
        if len(bad):
            k = int(bad[0])
            raise ValueError(f"'{self.filename}': population variant #{k} (INS at pos {int(t['v_pos'][k])}) has svlen "
                             f"{int(t['v_svlen'][k])}: combine_pctseq divides by it - not a usable population file")

    def lists_of(self, contig_no, pos, type_no) -> np.ndarray:
        """List number (-1: none) of every query: `contig_no` / `type_no` number the table's `contigs` / `types` (-1: not in the
        file), the block key is `str(int(pos / snf_block_size) * snf_block_size)`."""
        t = self.table()
        bs = int(self.config.snf_block_size)
        contig_no, type_no = np.asarray(contig_no, np.int64), np.asarray(type_no, np.int64)
        start = np.trunc(np.asarray(pos, np.float64) / bs).astype(np.int64) * bs
        ok = (contig_no >= 0) & (type_no >= 0) & (start >= 0) & (start < (1 << 40))
        key = (np.where(ok, contig_no, 0) << 44) | (np.where(ok, start, 0) << 4) | np.where(ok, type_no, 0)
        keys = t["keys"]
        if len(keys) == 0:
            return np.full(len(key), -1, np.int32)
        at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        return np.where(ok & (keys[at] == key), t["key_list"][at], -1).astype(np.int32)

    def get_population_AF_batch(self, calls_or_columns, config=None, device: int = 0):
        """`get_population_AF` for many calls in ONE launch.  `calls_or_columns`: a sequence of calls (`contig`, `pos`, `svlen`,
        `svtype`, `alt`), or columns - a dict with `list` (from `lists_of`), `pos`, `svlen` (int32 per query), `alt_off` (int64,
        n + 1) and `alt_pool` (uint8; only the ALT of a query against an insertion list is read).  Returns `(af, size)`: float64
        (the variant's AF rounded to 5 places; NaN where nothing matched - the reference's None) and int64 (0 there)."""
        config = config or self.config
        self._check_alignable(config)
        t = self.table()
        if isinstance(calls_or_columns, dict):
            q = calls_or_columns
        else:
            calls = list(calls_or_columns)
            alts = [_alt_bytes(c.alt) if c.svtype == "INS" else b"" for c in calls]
            alt_off = np.zeros(len(calls) + 1, np.int64)
            if calls:
                np.cumsum(np.fromiter((len(a) for a in alts), np.int64, len(alts)), out=alt_off[1:])
            pos = np.asarray([c.pos for c in calls], np.int64)
            q = dict(list=self.lists_of([t["contigs"].get(c.contig, -1) for c in calls], pos, [t["types"].get(c.svtype, -1) for c in calls]),
                     pos=pos, svlen=np.asarray([c.svlen for c in calls], np.int64), alt_off=alt_off,
                     alt_pool=np.frombuffer(b"".join(alts) + b"\0", np.uint8))
        n = len(q["alt_off"]) - 1
        if n <= 0:
            return np.zeros(0, np.float64), np.zeros(0, np.int64)
        best, _ = lib.population_match_batch(config, t, q, device=device)
        hit = best >= 0
        at = np.where(hit, best, 0)
        if len(t["af"]) == 0:
            return np.full(n, np.nan), np.zeros(n, np.int64)
        return np.where(hit, t["af"][at], np.nan), np.where(hit, t["size"][at], 0).astype(np.int64)

    def get_population_AF(self, svcall, device: int = 0):
        """(population AF rounded to 5 places, genotyped samples) of the best-matching variant, or None (snfp.py:131-155): a batch
        of one."""
        af, size = self.get_population_AF_batch([svcall], device=device)
        return None if af[0] != af[0] else (float(af[0]), int(size[0]))


class PopulationWriter:
    """`--dev-population-snf`: the merged calls of a merge as a population SNF.  `add_task` takes a task's calls in EMISSION order
    (before the sort by position and before the VCF writer touches them) and writes the task's part the way
    `CombineResultTmpFilePopulationSNF.finalize` does (result.py:266-277: `store` every call, `write_and_index`); `finish` is the main
    program's `write_results` (sniffles:565-568) and returns the number of variants written (calls with too few genotyped samples
    are dropped: `dev_population_min_gt`)."""

    def __init__(self, path: str, config):
        self.path, self.config = path, config
        self.out = PopulationSNF(config, open(path, "wb"), filename=path)

    def add_task(self, task_id: int, contig: str, calls) -> int:
        name = f"{self.path}.tmp_{task_id}.snf"
        part = PopulationSNF(self.config, open(name, "wb"), filename=name)
        stored = sum(1 for c in calls if part.store(c))
        part.write_and_index()
        part.close()
        self.out.add_result(snf.SNFPart(task_id=task_id, contig=contig, snf_filename=name, snf_index=part.get_index(),
                                        snf_total_length=part.get_total_length(), snf_candidate_count=stored, coverage_average_total=0.0))
        return stored

    def finish(self, contigs) -> int:
        try:
            return self.out.write_results(self.config, contigs)
        finally:
            self.out.close()


# ---- the merge's side: which population file, and the two INFO entries -------------------------------------------------------------
_OPENED = {}      # (real path, mtime, size, block size) -> PopulationSNF: a merge of many tasks / calls opens the file once


def population_of(config) -> Optional[PopulationSNF]:
    """`config.combine_population` as an opened `PopulationSNF` (None: no population).  The option may be the object itself - the
    reference's `CombineTask.execute` replaces the path by it (parallel.py:454-455) - or a path; the caller's config is left as
    it is: a file is opened once per process and state of the file (path, time stamp, size) and its table kept."""
    pop = getattr(config, "combine_population", None)
    if not pop:
        return None
    if isinstance(pop, PopulationSNF):
        return pop
    path = os.path.realpath(os.fspath(pop))
    st = os.stat(path)
    key = (path, st.st_mtime_ns, st.st_size, int(config.snf_block_size))
    opened = _OPENED.get(key)
    if opened is None:
        for k in [k for k in _OPENED if k[0] == path]:
            del _OPENED[k]
        opened = _OPENED[key] = PopulationSNF.open(path, config)
        opened.table()
        opened.close()
    return opened


def info_values(af, size) -> tuple:
    """The two `info` entries of a call with the reference's types (sv.py:475-479): `(round(af, 5), genotyped count)`, or the two
    ints `(0, 0)` when nothing matched."""
    return (0, 0) if af != af else (float(af), int(size))


def annotate_calls(calls, config, device: int = 0) -> None:
    """`POPULATION_AF` / `POPULATION_SIZE` of merged calls (sv.py:475-479), all calls in one launch."""
    pop = population_of(config)
    if pop is None or not calls:
        return
    af, size = pop.get_population_AF_batch(calls, config=config, device=device)
    for c, a, s in zip(calls, af.tolist(), size.tolist()):
        a, s = info_values(a, s)
        c.set_info("POPULATION_AF", a)
        c.set_info("POPULATION_SIZE", s)
