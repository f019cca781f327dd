"""TEST HELPER: a plain restatement of the reference's population lookup - `PopulationVariant.match` (snfp.py:91-107) and the
search loop of `PopulationSNF.get_population_AF` (snfp.py:131-155) - over lists of simple records, with the distances taken from the
exact DP of the C oracle (`oracle.edit_distance`).  The directed cases of tests/test_population_match.py hold
`lib.population_match_batch` against it; `test_restatement_agrees_with_the_reference` holds IT against the unmodified reference.
Also here: the packing of such lists into the CSR the entry point takes."""
import math
from collections import namedtuple

import numpy as np

V = namedtuple("V", "pos svlen alt svtype", defaults=("INS",))     # a population variant, or a call (the same four fields are read)


def edit_distance(a: str, b: str) -> int:
    import oracle
    return int(oracle.edit_distance(a.encode("latin-1"), b.encode("latin-1")))


def match(v, call, cfg, dist_fn=edit_distance, counters=None):
    """snfp.py:91-107, statement for statement."""
    dist = abs(v.pos - call.pos) + abs(abs(v.svlen) - abs(call.svlen))
    minlen = float(min(abs(v.svlen), abs(call.svlen)))
    if dist > cfg.combine_match * math.sqrt(minlen) or dist > cfg.combine_match_max:
        return None
    limit = cfg.combine_pctseq
    if v.svtype == "INS" and limit:
        if counters is not None:
            counters["gate_pairs"] += 1
        distance = dist_fn(v.alt, call.alt)
        if (v.svlen - distance) / v.svlen <= limit:
            return None
    return dist


def best_of(variants, call, cfg, dist_fn=edit_distance, counters=None):
    """The loop of snfp.py:139-153: (index of the best variant or -1, its dist or 0)."""
    best_dist, best = None, -1
    for k, v in enumerate(variants):
        dist = match(v, call, cfg, dist_fn, counters)
        if dist is not None and (best_dist is None or dist < best_dist):
            best_dist, best = dist, k
    return best, (0 if best < 0 else best_dist)


def reference(lists, queries, cfg, dist_fn=edit_distance):
    """`lists`: list of lists of V; `queries`: (call V, list number or -1).  Returns (best: index over ALL variants or -1, dist,
    counters): gate_pairs = (query, INS variant) pairs that pass the positional gate while the sequence gate is on, ins_answers =
    queries answered by an INS variant while it is on."""
    base = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    best, dist = [], []
    counters = dict(gate_pairs=0, ins_answers=0)
    for call, li in queries:
        b, d = (-1, 0) if li < 0 else best_of(lists[li], call, cfg, dist_fn, counters)
        if b >= 0 and cfg.combine_pctseq and lists[li][b].svtype == "INS":
            counters["ins_answers"] += 1
        best.append(-1 if b < 0 else int(base[li]) + b)
        dist.append(d)
    return np.asarray(best, np.int32), np.asarray(dist, np.int32), counters


def _pool(strs):
    off = np.zeros(len(strs) + 1, np.int64)
    if strs:
        np.cumsum([len(s) for s in strs], out=off[1:])
    return off, np.frombuffer("".join(strs).encode("latin-1") + b"\0", np.uint8)


def pack(lists, queries):
    """(table, queries) dicts of `lib.population_match_batch`.  A list is an insertion list when its variants are INS."""
    flat = [v for x in lists for v in x]
    v_off, v_pool = _pool([v.alt for v in flat])
    table = dict(list_off=np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64),
                 list_is_ins=np.asarray([bool(x) and x[0].svtype == "INS" for x in lists], np.uint8),
                 v_pos=np.asarray([v.pos for v in flat], np.int32), v_svlen=np.asarray([v.svlen for v in flat], np.int32),
                 v_alt_off=v_off, v_alt_pool=v_pool)
    q_off, q_pool = _pool([c.alt for c, _ in queries])
    q = dict(pos=np.asarray([c.pos for c, _ in queries], np.int32), svlen=np.asarray([c.svlen for c, _ in queries], np.int32),
             list=np.asarray([li for _, li in queries], np.int32), alt_off=q_off, alt_pool=q_pool)
    return table, q
