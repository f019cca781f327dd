"""TEST INFRASTRUCTURE ONLY - the ALT consensus (`consensus.novel_from_reads` of the reference) restated in plain Python, with a trace.

`novel_from_reads(best, others, klen, skip, skip_repetitive)` returns `(string, trace)`: the string the reference returns for the same
arguments and one tuple per decision taken, holding the integers that were compared:

    ("shift", i, j)          a sampled k-mer of an other read at j is an anchor of the best read at i: dropped iff |i - j| > klen
    ("chain", i, last_i)     ... and, after the first accepted anchor, dropped iff i <= last_i
    ("first", i, j)          the first accepted anchor: i leading gap columns iff j > 0
    ("clip", c + fwd_j, L)   every later accepted anchor: c columns written so far, fwd_j = j - last_j; clipped iff c + fwd_j > L
    ("seg", m, n)            a segment with fwd_i == fwd_j > 0: m of its offsets 1 .. n agree, copied iff 2 * m >= n
    ("run", ident, length)   a maximal run of copied columns: kept iff 2 * ident > length and ident > 5
    ("span", span, L)        once per other read: kept iff 5 * span > L
    ("vote", n, maxal, top, runner, top_char, best_char)
                             once per column with at least one vote: n votes of kept reads, maxal = 1 + kept reads; the column is
                             voted on iff n >= 2 and 4 * n >= maxal, and replaced by top_char iff top - runner >= 3 (counts of the two
                             most common characters among [best_char] + votes, ordered by (count, char) descending; runner 0 when
                             there is one character only, in which case nothing is replaced)

Integers only.  The reference compares quotients of Python floats with 0.5, 0.2 and 0.25; for the magnitudes that can occur (all
operands below 2^16) the integer forms above decide identically: a correctly rounded quotient m / n that is not exactly the
threshold differs from it by at least 1 / (5 * 65536), far more than half an ulp, 0.5 and 0.25 are exact doubles, and the double 0.2
is the correctly rounded 1 / 5, which is also what span / L gives when 5 * span == L - so `> 0.2` is false exactly there.
tests/test_consensus_thresholds.py checks both the quotient claim (exhaustively over the small operands the cases use) and the
strings (against the reference itself, over every recorded, generated and directed problem).

Nothing here is taken from the reference's text: it is the project's own account of the rule, like tests/genotype_ref.py.
A sequence is a str of single-byte characters; '-' inside a read is a gap, as in the reference."""


def sampled(seq, klen, step):
    """Sampled k-mer positions of a read: 0, step, ... below len(seq) - klen (the last k-mer of a read is never sampled)."""
    return range(0, len(seq) - klen, step)


def anchor_table(best, klen, step):
    """k-mer -> position for the k-mers met exactly once among the sampled positions of the best read."""
    first, seen_twice = {}, set()
    for i in sampled(best, klen, step):
        k = best[i:i + klen]
        if k in seen_twice:
            continue
        if k in first:
            del first[k]
            seen_twice.add(k)
        else:
            first[k] = i
    return first


def align_row(best, read, klen, skip, table, trace):
    """One other read against the anchors: (row of len(best) characters with '-' for gaps, span)."""
    L = len(best)
    row = []
    have, last_i, last_j, span = False, 0, 0, 0
    for j in sampled(read, klen, skip):
        i = table.get(read[j:j + klen])
        if i is None:
            continue
        trace.append(("shift", i, j))
        if abs(i - j) > klen:
            continue
        if have:
            trace.append(("chain", i, last_i))
            if i <= last_i:
                continue
            fwd_i, fwd_j = i - last_i, j - last_j
            trace.append(("clip", len(row) + fwd_j, L))
            if len(row) + fwd_j > L:
                fwd_j = L - len(row)
            if fwd_i == fwd_j and fwd_j > 0:
                n = j - last_j
                span += n
                m = sum(1 for o in range(1, n + 1) if read[last_j + o] == best[last_i + o])
                trace.append(("seg", m, n))
                row += list(read[last_j:last_j + fwd_j]) if 2 * m >= n else ["-"] * fwd_j
            else:
                row += ["-"] * fwd_j
        else:
            trace.append(("first", i, j))
            if j > 0:
                row = ["-"] * i
        have, last_i, last_j = True, i, j
    row += ["-"] * (L - len(row))
    # runs of copied columns
    h = 0
    while h < L:
        if row[h] == "-":
            h += 1
            continue
        h0, ident = h, 0
        while h < L and row[h] != "-":
            ident += row[h] == best[h]
            h += 1
        trace.append(("run", ident, h - h0))
        if not (2 * ident > h - h0 and ident > 5):
            row[h0:h] = ["-"] * (h - h0)
    trace.append(("span", span, L))
    return row, span


def novel_from_reads(best, others, klen, skip, skip_repetitive=None):
    skip_repetitive = skip if skip_repetitive is None else skip_repetitive
    if skip < 1 or skip_repetitive < 1:
        raise ValueError("a sampling step of 0")
    trace = []
    L = len(best)
    table = anchor_table(best, klen, skip_repetitive)
    kept = []
    for read in others:
        row, span = align_row(best, read, klen, skip, table, trace)
        if 5 * span > L:
            kept.append(row)
    maxal = 1 + len(kept) if L else 1
    out = []
    for q in range(L):
        votes = [r[q] for r in kept if r[q] != "-"]
        b = best[q]
        if votes:
            counts = {}
            for c in [b] + votes:
                counts[c] = counts.get(c, 0) + 1
            order = sorted(((n, c) for c, n in counts.items()), reverse=True)
            top, top_char = order[0]
            runner = order[1][0] if len(order) > 1 else 0
            trace.append(("vote", len(votes), maxal, top, runner, top_char, b))
            if len(votes) >= 2 and 4 * len(votes) >= maxal and len(order) > 1 and top - runner >= 3:
                b = top_char
        out.append(b)
    return "".join(out), trace
