"""The pairs and the probe of tests/test_edit_distance_edges.py: string pairs at the form edges of the bit-parallel Myers kernels
(every length and cut-off derived from the literals tests/size_classes.py reads out of snf_myers.h / snf_myers.hip / snf_combine.hip),
and merge problems that read the predicate d(A, B) <= k out of the merge kernel.

The probe.  An INS problem with combine_pctseq = 0.5, every position equal and every length (the group's len_mean, the candidates'
svlen) equal to 2k + 2 passes the positional gates with distance 0 and accepts iff (2k + 2 - d) / (2k + 2) > 0.5, i.e. iff d <= k -
all of it exact in binary floating point - so the kernel's cut-off search yields kmax = k and the candidate B joins A's group iff
d(A, B) <= k.  Two forms: "group" - A is the ALT of an initial group (read from g_alt_pool), B the one candidate; "pair" - no initial
group, candidates A (support 5) and B (support 3): A founds the group, its ALT is read from alt_pool."""
import functools

import numpy as np

import size_classes as sc
from sniffles_amd import abi
from sniffles_amd.soa import SVT

E = sc.ed_thresholds()
BLOCK = sc.WAVE                                  # pattern rows of a Myers block: one 64-bit word
GROUP = sc.GROUP                                 # text columns of one step of ed_wave_pair_k_acgt8: one 8-byte word
THREAD_MAX = BLOCK * E["thread_blocks"]          # longest pattern of the thread form of ed_batch (512)
ROUND = sc.WAVE * 8                              # bytes one round of the identical-strings shortcut compares (64 lanes x 8)
ROT = BLOCK * E["band_pattern_blocks"]           # longest pattern whose blocks all have a lane of their own (4032)
BAND_EDGE = BLOCK * (E["band_blocks"] - 2)       # dl + 2 kk from which the band no longer fits the wave (3904)
PROBE_PCTSEQ = 0.5
FORMS = ("group", "pair")
OTHER = b"Nacgtn"                                # bytes outside {A, C, G, T}


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8)) if n else b""


def mutated(rng, a, n_sub, n_ins, alphabet=b"ACGT"):
    """a with n_sub bytes replaced and n_ins bytes inserted (len + n_ins)."""
    b = bytearray(a)
    for _ in range(n_sub if b else 0):
        b[int(rng.integers(0, len(b)))] = int(rng.choice(list(alphabet)))
    for _ in range(n_ins):
        b.insert(int(rng.integers(0, len(b) + 1)), int(rng.choice(list(alphabet))))
    return bytes(b)


def sprinkle(rng, s, count, alphabet=OTHER):
    b = bytearray(s)
    for p in rng.integers(0, len(b), count) if b else []:
        b[int(p)] = int(rng.choice(list(alphabet)))
    return bytes(b)


SHORT_M = sorted({0, 1, 2} | set(sc.around(GROUP, BLOCK, 2 * BLOCK, THREAD_MAX)))       # 0 1 2 7 8 9 63 64 65 127 128 129 511 512 513
SHORT_DL = [0, 1] + sc.around(GROUP)                                                    # 0 1 7 8 9


@functools.lru_cache(maxsize=None)
def short_pairs():
    """[(kind, A, B)]: every m x (n - m) of the ladders above in three alphabets - "acgt" (pattern and text over ACGT: acgt8<true>),
    "text_other" (a few N / lower-case bytes in the TEXT: acgt8<false>), "planes" (an N in the PATTERN: bit-plane form) - plus the
    symbolic ALTs.  The pattern is the shorter string (A when equal); which side it is on alternates."""
    rng = np.random.default_rng(20)
    out = [("symbolic", b"<INS>", b"<DEL>"), ("symbolic", b"<DEL>", b"<DEL>"), ("symbolic", b"<DEL>", b"<INS>"), ("symbolic", b"<INS>", b"<INS>")]
    for m in SHORT_M:
        for dl in SHORT_DL:
            for kind in ("acgt", "text_other", "planes"):
                p = rnd(rng, m)
                t = mutated(rng, p, int(rng.integers(0, 2 + m // 10)), dl)
                if kind == "text_other":
                    t = sprinkle(rng, t, 3)
                    if m == len(t):                       # equal lengths: A is the pattern, so it goes first
                        out.append((kind, p, t))
                        continue
                elif kind == "planes":
                    if m == 0:
                        continue
                    p = sprinkle(rng, p, 2, b"N")
                    t = sprinkle(rng, t, 1)
                out.append((kind, p, t) if (m + dl) % 2 == 0 else (kind, t, p))
    return out


def short_ks(a, b, d):
    """0, d - 1, d, d + 1, n - m - 1 and max(m, n), none below 0."""
    return sorted({max(0, k) for k in (0, d - 1, d, d + 1, abs(len(a) - len(b)) - 1, max(len(a), len(b)))})


SHORTCUT_M = [1, GROUP - 1, GROUP, GROUP + 1, ROUND, ROUND + 1, ROUND + GROUP, 2 * ROUND + GROUP - 1]     # 1 7 8 9 512 513 520 1031


@functools.lru_cache(maxsize=None)
def shortcut_pairs():
    """[(A, B, d)]: equal lengths around the 8-byte words and the 512-byte rounds of the identical-strings shortcut; B is A itself
    (d = 0, another object) or A with one substitution (d = 1) at the first / last byte of a word, of a round, of the tail."""
    rng = np.random.default_rng(21)
    out = []
    for m in SHORTCUT_M:
        a = rnd(rng, m)
        out.append((a, bytes(bytearray(a)), 0))
        for p in sorted({0, GROUP - 1, GROUP, ROUND - 1, ROUND, m - GROUP, m - 1}):
            if 0 <= p < m:
                b = bytearray(a)
                b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + int(rng.integers(0, 3))) % 4]
                out.append((a, bytes(b), 1))
    return out


def constructed(m, dl, d, lo=b"AC", hi=b"GT", seed=0):
    """(A, B) with len(A) = m, len(B) = m + dl and d(A, B) = d by construction: A over `lo`; B is A with a block of d - dl bytes replaced
    by bytes over `hi` and dl more bytes over `hi` appended.  No byte of `hi` matches anything in A, so each costs at least one edit,
    and substituting / inserting them is an alignment of exactly that cost."""
    rng = np.random.default_rng([22, m, dl, d, seed])
    s = d - dl
    assert 0 <= s <= m and not set(lo) & set(hi)
    a = rnd(rng, m, lo)
    off = min(BLOCK - GROUP - 1, m - s)
    return a, a[:off] + rnd(rng, s, hi) + a[off + s:] + rnd(rng, dl, hi)


def near(m, dl, planes, seed=0):
    """A near-identical pair of m and m + dl bytes (about 40 edits); planes: an N in both (bit-plane form)."""
    rng = np.random.default_rng([23, m, dl, int(planes), seed])
    a = rnd(rng, m)
    if planes:
        a = sprinkle(rng, a, 3, b"N")
    b = bytearray(mutated(rng, a, 24, 8 + dl))
    for _ in range(8):
        del b[int(rng.integers(0, len(b)))]
    return a, bytes(b)


ALPHABETS = {"acgt": (b"AC", b"GT"), "planes": (b"ACN", b"GT")}
WIDE_M = [ROT + 1, ROT + BLOCK + 4]                                       # 4033, 4100: more than 63 blocks
WIDE_K = [BAND_EDGE - 2, BAND_EDGE - 1, BAND_EDGE, BAND_EDGE + 1]         # 3902 .. 3905: both sides of the band rule for n - m = 0 and 1
ROTATING_M = [ROT, ROT + 1, ROT + BLOCK, ROT + BLOCK + 1, ROT + 2 * BLOCK, ROT + 2 * BLOCK + 1]      # 63 | 64 | 65 | 66 blocks


def wide_cases(m, alphabet="acgt"):
    """[(A, B, k)] around the band-fit edge for patterns of more than 63 blocks: k x d in {k - 1, k, k + 1} with d known by
    construction, and a near-identical pair at the same k."""
    lo, hi = ALPHABETS[alphabet]
    out = []
    for dl in (0, 1):
        a_n, b_n = near(m, dl, alphabet == "planes")
        for k in WIDE_K:
            for d in (k - 1, k, k + 1):
                a, b = constructed(m, dl, d, lo, hi)
                out.append((a, b, k))
            out.append((a_n, b_n, k))
    return out


def filler(i):
    """A short problem's pair for between two long ones: maxlen carry_min_len (4000: eight carry bytes) at i = 1 of every eight,
    carry_min_len + 1 (4001: a carry row of its own) at i = 5, five bytes otherwise; near-identical, so the band is narrow."""
    n = {1: E["carry_min_len"], 5: E["carry_min_len"] + 1}.get(i % 8, 5)
    a, b = near(n, 0, False) if n > 100 else (b"ACGTA", b"ACTTA")
    assert max(len(a), len(b)) == n
    return a, b, 60


def probe(a, b, k, form, keep, ln=None):
    """(struct, out_group, out_group if d(a, b) <= k, out_group otherwise) of one probe problem.  ln: another length than 2k + 2 for
    len_mean and svlen (a problem at another combine_pctseq: B joins iff (ln - d) / ln exceeds it)."""
    if ln is None:
        assert k >= 0
        ln = 2 * k + 2
    empty = dict(pos_mean=[], len_mean=[], mate_mean=[], size=[], mate_contig=[], alts=[], samples=[])
    if form == "group":
        cands = dict(pos=[1000], svlen=[ln], support=[3], sample_id=[1], mate_contig=[0], mate_ref_start=[0], alts=[b])
        groups = dict(pos_mean=[1000.0], len_mean=[float(ln)], mate_mean=[0.0], size=[1], mate_contig=[0], alts=[a], samples=[[0]])
        yes, no = [0], [1]
    else:
        cands = dict(pos=[1000, 1000], svlen=[ln, ln], support=[5, 3], sample_id=[0, 1], mate_contig=[0, 0], mate_ref_start=[0, 0], alts=[a, b])
        groups = empty
        yes, no = [0, 0], [0, 1]
    q, out = abi.combine_problem(SVT["INS"], cands, groups, 2, keep)
    return q, out, yes, no
