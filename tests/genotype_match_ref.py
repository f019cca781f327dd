"""The match of `GenotypeTask.execute` (reference parallel.py:300-369) in plain Python, restated per target - the rule
`snf_genotype_match_batch` implements (include/sniffles_amd.h), over the same column tables.

    candidates / targets: dicts of equally long int lists svtype (SNF_* code, -1 for a type outside sv.TYPES), pos, svlen, mate_contig

The reference walks the candidates and lets each look into the 5-kb bin of its own position, where the targets were filed (a target
within 500 bp of a bin edge also into the neighbour); here every target looks for its candidates, which is the same relation."""
import math

BINSIZE, BINEDGE = 5000, 500
INS, DEL, DUP, INV, BND = range(5)
SINGLE_LEFT, SINGLE_RIGHT = 5, 6
TYPE_CODES = {"INS": INS, "DEL": DEL, "DUP": DUP, "INV": INV, "BND": BND, "SINGLE_LEFT": SINGLE_LEFT, "SINGLE_RIGHT": SINGLE_RIGHT}


def code(svtype: str) -> int:
    return TYPE_CODES.get(svtype, -1)


def visible_bins(pos: int) -> list:
    b0 = int(pos / BINSIZE)
    bins = [b0]
    if pos % BINSIZE < BINEDGE:
        bins.append(b0 - 1)
    if pos % BINSIZE > BINSIZE - BINEDGE:
        bins.append(b0 + 1)
    return bins


def sees(cpos: int, tpos: int) -> bool:
    return cpos >= 0 and int(cpos / BINSIZE) in visible_bins(tpos)


def gates(ttype, tpos, tsvlen, tmate, cpos, csvlen, cmate, cfg):
    """(dist, ok) of a target / candidate pair of the same type, whatever the bins say."""
    if ttype == BND:
        dist = abs(tpos - cpos)
        return dist, dist <= cfg.cluster_merge_bnd and cmate == tmate
    dist = abs(tpos - cpos) + abs(abs(tsvlen) - abs(csvlen))
    minlen = float(min(abs(tsvlen), abs(csvlen)))
    return dist, minlen > 0 and dist <= cfg.combine_match * math.sqrt(minlen) and dist <= cfg.combine_match_max


def pair(ttype, tpos, tsvlen, tmate, ctype, cpos, csvlen, cmate, cfg):
    """(takes part and sees the target, dist, passes the gates) of one target / candidate pair."""
    if not (INS <= ttype <= BND) or ctype != ttype or not sees(cpos, tpos):
        return False, None, False
    dist, ok = gates(ttype, tpos, tsvlen, tmate, cpos, csvlen, cmate, cfg)
    return True, dist, ok


def match(candidates: dict, targets: dict, cfg):
    """(best: candidate index or -1 per target, dist: its distance or 0)."""
    by_key = {}
    for i, (t, p) in enumerate(zip(candidates["svtype"], candidates["pos"])):
        if INS <= t <= BND and p >= 0:
            by_key.setdefault((t, int(p / BINSIZE)), []).append(i)
    best, dist = [], []
    for tt, tp, tl, tm in zip(targets["svtype"], targets["pos"], targets["svlen"], targets["mate_contig"]):
        b, d = -1, None
        if INS <= tt <= BND:
            for bin_ in visible_bins(tp):
                for i in by_key.get((tt, bin_), ()):
                    _, dd, ok = pair(tt, tp, tl, tm, candidates["svtype"][i], candidates["pos"][i], candidates["svlen"][i], candidates["mate_contig"][i], cfg)
                    if ok and (d is None or (dd, i) < (d, b)):
                        b, d = i, dd
        best.append(b)
        dist.append(0 if d is None else d)
    return best, dist


def tables_from_records(cand_records, specs):
    """Column tables of a golden case: the reference's candidate records (id, svtype, pos, svlen, bnd) and the target specs of
    tests/genotype_util.py.  Mate contigs are numbered by name over both."""
    names = {}

    def mate(bnd):
        return -1 if not bnd else names.setdefault(bnd[0], len(names))
    cands = dict(svtype=[code(c["svtype"]) for c in cand_records], pos=[c["pos"] for c in cand_records], svlen=[c["svlen"] for c in cand_records],
                 mate_contig=[mate(c.get("bnd")) if c["svtype"] == "BND" else -1 for c in cand_records])
    targets = dict(svtype=[code(t["svtype"]) for t in specs], pos=[t["pos"] for t in specs], svlen=[t["svlen"] for t in specs],
                   mate_contig=[mate(t["bnd"]) if t["svtype"] == "BND" else -1 for t in specs])
    return cands, targets
