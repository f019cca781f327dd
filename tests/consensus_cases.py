"""TEST INFRASTRUCTURE ONLY - directed problems ON the decision thresholds of the ALT consensus (consensus.py:280-394).

Every case is a dictionary `name, best, others, klen, skip, expect_trace, diff` built deterministically from a seeded best read in which
every k-mer (at every position, not only the sampled ones) is unique and which holds no 'AAA' - so no anchor is taboo by accident and a
run of 'A' shares no k-mer with it.  `expect_trace`: tuples of tests/consensus_ref.py that must occur; `forbid`: predicates no tuple may
satisfy; `diff`: the columns in which the consensus must differ from the best read (None: only that `must_change` are among them).  The
builder asserts all of that on the restatement before a case is handed out: a case that has drifted off its edge fails as such, whatever
the kernels do.  The cases of one threshold come in pairs whose `diff` differs: at least four identical other reads carry a base the
best read does not have inside the affected columns, so the decision shows in the output - except where the rule itself hides it
(listed in DESIGN.md: `len(al) < 2`, the tie order, the clip, runs made of anchors only).

The expected strings of the reference are in tests/golden/consensus_thresholds.json.gz (oracle/make_golden.py consensus_thresholds)."""
import functools
import hashlib

import numpy as np

import consensus_ref as cr

NEXT = {"A": "C", "C": "G", "G": "T", "T": "A"}


def unique_read(seed, L, klen):
    """Random ACGT of length L, every k-mer unique, no 'AAA' (depth-first with a seeded order of the bases)."""
    rng = np.random.default_rng([20261020, seed])
    seq, used, tried = [], set(), [None] * L
    while len(seq) < L:
        q = len(seq)
        if tried[q] is None:
            tried[q] = ["ACGT"[k] for k in rng.permutation(4)]
        placed = False
        while tried[q]:
            c = tried[q].pop()
            if c == "A" and seq[-2:] == ["A", "A"]:
                continue
            k = "".join(seq[q - klen + 1:] + [c]) if q >= klen - 1 else None
            if k is not None and k in used:
                continue
            seq.append(c)
            if k is not None:
                used.add(k)
            placed = True
            break
        if not placed:      # back up one base
            tried[q] = None
            assert q > 0
            if q >= klen:
                used.discard("".join(seq[q - klen:q]))
            seq.pop()
    s = "".join(seq)
    assert len({s[i:i + klen] for i in range(L - klen + 1)}) == L - klen + 1 and "AAA" not in s
    return s


def put(s, changes):
    """s with {position: character} applied."""
    t = list(s)
    for q, c in changes.items():
        t[q] = c
    return "".join(t)


def subs(s, positions):
    """s with the bases at `positions` replaced by the next base (A -> C -> G -> T -> A): never equal to the original."""
    return put(s, {q: NEXT[s[q]] for q in positions})


def unrelated(L):
    """An other read none of whose k-mers occurs in a best read of this module: never an anchor, never kept, never counted."""
    return "A" * L


def problem_sha(p) -> str:
    h = hashlib.sha256()
    for s in [p["best"]] + list(p["others"]):
        h.update(s.encode("latin-1")); h.update(b"|")
    h.update(repr((p["klen"], p["skip"])).encode())
    return h.hexdigest()


def _case(out, name, best, others, klen, skip, expect, diff, forbid=(), must_change=(), cluster=True):
    got, trace = cr.novel_from_reads(best, others, klen, skip, skip)
    seen = set(trace)
    for t in expect:
        assert t in seen, (name, "the case has left its edge: no", t, sorted(x for x in seen if x[0] == t[0])[:40])
    for f in forbid:
        assert not [t for t in trace if f(t)], (name, "a tuple the case excludes", [t for t in trace if f(t)][:5])
    cols = [q for q in range(len(best)) if got[q] != best[q]]
    if diff is not None:
        assert cols == sorted(diff), (name, cols, sorted(diff))
    assert set(must_change) <= set(cols), (name, cols)
    assert 4 <= klen <= 7 and 1 <= skip <= 7 and len(best) <= 384
    assert not any(c["name"] == name for c in out)
    # cluster: every read as long as the best one - the problem can be phrased as an INS cluster of a whole pass
    cluster = cluster and len(others) >= 2 and all(len(o) == len(best) for o in others)
    out.append(dict(name=name, best=best, others=list(others), klen=klen, skip=skip, expect_trace=list(expect), diff=cols,
                    restated=got, cluster=cluster))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    B6 = unique_read(1, 120, 6)      # klen 6, skip 3
    B4 = unique_read(2, 100, 4)      # klen 4, skip 4
    B43 = unique_read(3, 100, 4)     # klen 4, skip 3
    B7 = unique_read(4, 120, 7)      # klen 7, skip 3
    B41 = unique_read(5, 80, 4)      # klen 4, skip 1
    r = lambda a, b: list(range(a, b))

    # ------------------------------------------------------------------ segment identity: 2 * m >= n
    # one segment between the intact anchors a and a + n, every sampled k-mer between them destroyed; offsets 1 .. klen - 1 and n agree
    # by construction (they lie in the anchors), the free positions a + klen .. a + n - 1 are substituted or left
    a = 30
    _case(out, "seg_6_of_12", B6, [subs(B6, r(a + 6, a + 12))] * 4, 6, 3, [("seg", 6, 12)], r(a + 6, a + 12))
    for m, keep in ((8, [a + 10, a + 13]), (9, [a + 10, a + 11, a + 13]), (10, [a + 10, a + 11, a + 13, a + 14])):
        sub = [q for q in r(a + 6, a + 18) if q not in keep]
        _case(out, f"seg_{m}_of_18", B6, [subs(B6, sub)] * 4, 6, 3, [("seg", m, 18)], sub if 2 * m >= 18 else [])
    for m, keep in ((7, [a + 10]), (8, [a + 10, a + 11])):
        sub = [q for q in r(a + 6, a + 15) if q not in keep]
        _case(out, f"seg_{m}_of_15", B6, [subs(B6, sub)] * 4, 6, 3, [("seg", m, 15)], sub if 2 * m >= 15 else [])

    # ------------------------------------------------------------------ run filter: 2 * ident > length and ident > 5
    # an isolated run: one copied segment between two segments of 12 that fail (4 of 12: their eight free positions substituted)
    for ident, sub in ((6, [36, 38]), (5, [36, 37, 38])):
        rd = subs(B4, r(24, 32) + sub + r(44, 52))
        _case(out, f"run_abs_{ident}_of_8", B4, [rd] * 4, 4, 4, [("seg", 4, 12), ("seg", ident, 8), ("run", ident, 8)], sub if ident > 5 else [])
    # six columns made of three adjacent anchors (30, 33, 36) between two failed segments of 9: kept, and every column agrees
    rd = subs(B43, r(25, 30) + r(40, 45))
    _case(out, "run_abs_6_of_6_anchors_only", B43, [rd] * 4, 4, 3, [("seg", 4, 9), ("seg", 3, 3), ("run", 6, 6)], [])
    for ident, sub in ((6, [36, 37, 38, 40, 41, 42]), (7, [36, 37, 40, 41, 42])):
        rd = subs(B4, r(24, 32) + sub + r(48, 56))
        _case(out, f"run_ratio_{ident}_of_12", B4, [rd] * 4, 4, 4, [("seg", ident, 12), ("run", ident, 12)], sub if 2 * ident > 12 else [])

    # ------------------------------------------------------------------ read filter: 5 * span > L
    # the other reads are the best read's first 30 (34) bases - last anchor at 24 (28), the span - and unrelated bases behind
    for L, span in ((116, 24), (120, 24), (124, 24), (119, 24), (121, 24), (120, 28), (121, 28), (140, 28), (141, 28)):
        best = unique_read(100 + L, L, 6)
        rd = subs(best[:span + 6] + unrelated(L - span - 6), [10])
        _case(out, f"span_{span}_of_{L}", best, [rd] * 4, 6, 4, [("span", span, L)], [10] if 5 * span > L else [])
    v58 = subs(B6, [58])
    one_anchor = put(unrelated(120), {48 + k: B6[48 + k] for k in range(6)})
    _case(out, "span_no_anchor_reads_do_not_count", B6, [v58] * 4 + [unrelated(120)] * 12, 6, 3, [("span", 0, 120)], [58],
          forbid=[lambda t: t[0] == "first" and t[1] != t[2]])
    _case(out, "span_one_anchor_reads_do_not_count", B6, [v58] * 4 + [one_anchor] * 12, 6, 3, [("first", 48, 48), ("span", 0, 120)], [58])

    # ------------------------------------------------------------------ the column vote
    # column x; voters carry a chosen byte there, `same` is the best read itself, `dash` has a failed segment (6 of 15) over columns
    # 51 .. 65: it is kept, counts in maxal and does not vote at x
    x = 58
    b = B6[x]
    X, Y = NEXT[b], NEXT[NEXT[b]]
    vote = lambda c: put(B6, {x: c})
    same, dash = B6, subs(B6, r(57, 66))
    top2 = lambda *cs: max(cs)
    _case(out, "vote_support_1", B6, [vote(X)], 6, 3, [("vote", 1, 2, 1, 1, top2(X, b), b)], [])
    _case(out, "vote_support_2", B6, [vote(X)] * 2, 6, 3, [("vote", 2, 3, 2, 1, X, b)], [])
    for d in (12, 11, 10):
        _case(out, f"vote_4_of_maxal_{5 + d}", B6, [vote(X)] * 4 + [dash] * d, 6, 3, [("seg", 6, 15), ("vote", 4, 5 + d, 4, 1, X, b)],
              [x] if 16 >= 5 + d else [])
    _case(out, "vote_margin_3_best_runner_up", B6, [vote(X)] * 4, 6, 3, [("vote", 4, 5, 4, 1, X, b)], [x])
    _case(out, "vote_margin_2_best_runner_up", B6, [vote(X)] * 4 + [same], 6, 3, [("vote", 5, 6, 4, 2, X, b)], [])
    _case(out, "vote_margin_3_best_runner_up_2", B6, [vote(X)] * 5 + [same], 6, 3, [("vote", 6, 7, 5, 2, X, b)], [x])
    _case(out, "vote_margin_3_third_base_runner_up", B6, [vote(X)] * 5 + [vote(Y)] * 2, 6, 3, [("vote", 7, 8, 5, 2, X, b)], [x])
    _case(out, "vote_margin_2_third_base_runner_up", B6, [vote(X)] * 5 + [vote(Y)] * 3, 6, 3, [("vote", 8, 9, 5, 3, X, b)], [])
    _case(out, "vote_tie_of_two_other_bases", B6, [vote(X), vote(Y)] * 4, 6, 3, [("vote", 8, 9, 4, 4, top2(X, Y), b)], [])
    _case(out, "vote_tie_then_margin_3", B6, [vote(X)] * 7 + [vote(Y)] * 4 + [same] * 3, 6, 3, [("vote", 14, 15, 7, 4, X, b)], [x])
    _case(out, "vote_top_is_the_best_base", B6, [same] * 5 + [vote(X)], 6, 3, [("vote", 6, 7, 6, 1, b, b)], [])
    _case(out, "vote_all_equal_to_the_best_base", B6, [same] * 4, 6, 3, [("vote", 4, 5, 5, 0, b, b)], [])
    _case(out, "vote_N_wins", B6, [vote("N")] * 4, 6, 3, [("vote", 4, 5, 4, 1, "N", b)], [x])
    xa = next(q for q in range(58, 90, 3) if B6[q] not in "A")      # (x = 1 mod 3: the dash read's failed segment starts 7 before it)
    ba = B6[xa]
    va = lambda c: put(B6, {xa: c})
    _case(out, "vote_lower_case_a_loses_to_A", B6, [va("A")] * 5 + [va("a")] * 2, 6, 3, [("vote", 7, 8, 5, 2, "A", ba)], [xa])
    _case(out, "vote_lower_case_a_is_not_A", B6, [va("A")] * 3 + [va("a")], 6, 3, [("vote", 4, 5, 3, 1, "A", ba)], [])
    _case(out, "vote_unrelated_reads_do_not_count", B6, [vote(X)] * 4 + [unrelated(120)] * 13, 6, 3, [("vote", 4, 5, 4, 1, X, b)], [x])

    # ------------------------------------------------------------------ anchors
    # the first anchor: gap columns in front of it only when j > 0
    # (reads that lose bases at one end get unrelated ones at the other: every read as long as the best one, so that the case can be an
    # INS cluster of a whole pass)
    _case(out, "first_anchor_j0_i_skip", B6, [v58[3:] + unrelated(3)] * 4, 6, 3, [("first", 3, 0)], [])
    _case(out, "first_anchor_j_skip_i0", B6, [unrelated(3) + v58[:-3]] * 4, 6, 3, [("first", 0, 3)], [58])
    # |i - j| <= klen on the sampling grid: klen itself when it is a multiple of skip, the next grid shift beyond it
    for nm, best, klen, skip, ok, no in (("k6s3", B6, 6, 3, 6, 9), ("k7s3", B7, 7, 3, 6, 9), ("k4s1", B41, 4, 1, 4, 5), ("k4s4", B4, 4, 4, 4, 8)):
        col = 58 if len(best) > 100 else 42
        vr = subs(best, [col])
        _case(out, f"shift_{nm}_j_ahead_{ok}", best, [unrelated(ok) + vr[:-ok]] * 4, klen, skip, [("shift", 0, ok), ("first", 0, ok)], [col])
        _case(out, f"shift_{nm}_j_ahead_{no}", best, [unrelated(no) + vr[:-no]] * 4, klen, skip, [("shift", 0, no), ("span", 0, len(best))], [],
              forbid=[lambda t: t[0] == "first"])
        # i ahead: the read lacks the first d bases and its own first base differs, so that its first anchor has j = skip > 0
        for d, hit in ((ok, True), (no, False)):
            rd = NEXT[vr[d]] + vr[d + 1:] + unrelated(d)
            _case(out, f"shift_{nm}_i_ahead_{d}", best, [rd] * 4, klen, skip,
                  [("shift", d + skip, skip)] + ([("first", d + skip, skip)] if hit else [("span", 0, len(best))]), [col] if hit else [],
                  forbid=[] if hit else [lambda t: t[0] == "first"])
    # the clip at L: a read that starts klen behind and, after 2 * klen inserted bases, runs klen ahead writes past column L
    rd = NEXT[v58[6]] + v58[7:90] + unrelated(12) + v58[90:]
    _case(out, "clip_L_plus_skip", B6, [rd] * 4, 6, 3, [("first", 9, 3), ("clip", 123, 120), ("clip", 120, 120)], None, must_change=[58])
    v42 = subs(B41, [42])
    rd = NEXT[v42[3]] + v42[4:60] + unrelated(6) + v42[60:]
    _case(out, "clip_L_plus_1", B41, [rd] * 4, 4, 1, [("first", 4, 1), ("clip", 81, 80), ("clip", 80, 80)], None, must_change=[42])
    # an insertion of skip bases in the middle: fwd_j != fwd_i, gap columns, everything behind it one step off the best read
    rd = v58[:90] + unrelated(3) + v58[90:]
    _case(out, "insertion_of_skip_in_the_middle", B6, [rd] * 4, 6, 3, [("shift", 90, 93), ("clip", 114, 120)], None, must_change=[58])
    # a k-mer of the other read that repeats the previous anchor: i == last_i
    # (the best read repeats three bases, 81 .. 83 at 84 .. 86, the other reads repeat them once more: their k-mer at 84 is the best
    # read's at 81, which their own k-mer at 81 was already) ... and one that falls behind it: i < last_i
    for src, nm in ((81, "equals"), (78, "is_below")):
        best = put(B6, {84 + k: B6[src + k] for k in range(3)})
        rd = put(subs(best, [58]), {87 + k: best[81 + k] for k in range(3)})
        _case(out, f"chain_i_{nm}_last_i", best, [rd] * 4, 6, 3, [("chain", 81, 78), ("chain", src, 81)], None, must_change=[58])
    # a k-mer twice on the sampling grid of the best read is no anchor; twice with one occurrence off the grid it still is
    twice = put(B6, {96 + k: B6[21 + k] for k in range(6)})
    _case(out, "kmer_twice_on_the_grid", twice, [subs(twice, [58])] * 4, 6, 3, [], [58], forbid=[lambda t: t[0] == "shift" and t[1] in (21, 96)])
    off = put(B6, {97 + k: B6[21 + k] for k in range(6)})
    _case(out, "kmer_twice_once_off_the_grid", off, [subs(off, [58])] * 4, 6, 3, [("shift", 21, 21)], [58])
    # other reads shorter than a k-mer, a k-mer long, one base longer (one sampled position), empty, longer than L + klen
    _case(out, "other_reads_of_odd_lengths", B6, [v58] * 3 + ["", B6[:5], B6[:6], B6[:7], v58 + unrelated(20)], 6, 3,
          [("first", 0, 0), ("span", 0, 120), ("vote", 4, 5, 4, 1, X, b)], [58])
    for L in (6, 7, 9, 10):     # 0, 1, 1 and 2 sampled positions
        _case(out, f"best_read_of_{L}", B6[:L], [B6[:L]] * 4, 6, 3, [("span", 3 if L == 10 else 0, L)] if L > 6 else [], [])
    _case(out, "no_other_reads", B6, [], 6, 3, [], [])
    _case(out, "one_other_read", B6, [v58], 6, 3, [("vote", 1, 2, 1, 1, top2(X, b), b)], [])

    # ------------------------------------------------------------------ the vote counters at their width
    # four 8-bit counters a column in one word (snf_wave_cons.h): 254 other reads - the most a LARGE call admits - agree on a base in
    # three columns; one vote more would carry into the next base's counter (code order A C T G), out of the word from G's
    Bc = unique_read(6, 200, 6)
    for z, c in enumerate("ACTG"):
        nb = "ACTG"[(z + 1) % 4]
        cols = [next(q for q in range(q0, q0 + 40) if Bc[q] not in (c, nb)) for q0 in (40, 100, 160)]
        rd = put(Bc, {q: c for q in cols})
        _case(out, f"counter_254_votes_{c}", Bc, [rd] * 254, 6, 3, [("vote", 254, 255, 254, 1, c, Bc[q]) for q in cols], cols)
        _case(out, f"counter_253_votes_{c}_and_1_{nb}", Bc, [rd] * 253 + [put(Bc, {q: nb for q in cols})], 6, 3,
              [("vote", 254, 255, 253, 1, c, Bc[q]) for q in cols], cols)
    cols = [next(q for q in range(q0, q0 + 40) if Bc[q] != "G") for q0 in (40, 100, 160)]
    _case(out, "counter_255_votes_G", Bc, [put(Bc, {q: "G" for q in cols})] * 255, 6, 3, [("vote", 255, 256, 255, 1, "G", Bc[q]) for q in cols], cols)
    # ... where the count itself decides (a column on which all 254 agree is won whatever a counter holds above 4): two bases share
    # the 254 votes with a margin of 2 or 4, both counters above 7 bits; and the most kept reads a LARGE call can have, 254, of
    # which 63 or 64 vote at the column (4 * votes against maxal = 255) while the others carry a failed segment there
    cB, cX, cY = Bc[100], NEXT[Bc[100]], NEXT[NEXT[Bc[100]]]
    for nx, ny in ((128, 126), (129, 125)):
        _case(out, f"counter_{nx}_votes_against_{ny}", Bc, [put(Bc, {100: cX})] * nx + [put(Bc, {100: cY})] * ny, 6, 3,
              [("vote", 254, 255, nx, ny, cX, cB)], [100] if nx - ny >= 3 else [])
    gap = subs(Bc, r(99, 108))      # 6 of 15 over columns 93 .. 107
    for nv in (63, 64):
        _case(out, f"counter_{nv}_votes_of_254_kept", Bc, [put(Bc, {100: cX})] * nv + [gap] * (254 - nv), 6, 3,
              [("seg", 6, 15), ("vote", nv, 255, nv, 1, cX, cB)], [100] if 4 * nv >= 255 else [])
    for p in out:       # the unrelated read really is unrelated to every best read
        kb = {p["best"][i:i + p["klen"]] for i in range(len(p["best"]) - p["klen"] + 1)}
        assert "A" * p["klen"] not in kb
    return out


# the class is moved without moving the decision: unrelated other reads appended until the call has this many
PADDINGS = {"large": 65, "rows": 255, "thread": 513}


def padded(p, n_others):
    """The case with unrelated reads appended up to n_others other reads (None when it has more already)."""
    if len(p["others"]) > n_others:
        return None
    q = dict(p)
    q["others"] = p["others"] + [unrelated(len(p["best"]))] * (n_others - len(p["others"]))
    return q
