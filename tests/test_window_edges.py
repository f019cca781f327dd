"""Directed cases for the window front end (snf_stage_window.h: w1_hist ... w6t_emit), the first thing every default pass runs.

The builders are in tests/window_cases.py, the literals come from size_classes.window_thresholds().  Every case is checked three ways:
(a) the layout it was planned for - width, window slots, occupied windows, largest window, windows of more than 64 leads, one launch
or two - is what the handle itself reports in its `[SNF_PROF] window front end` line (a case that no longer has the planned layout
fails, it does not test something else); (b) two run_pass calls and then call_candidates + finalize on one handle give the C oracle's
result, bit for bit (w2 must leave wcnt / wfill clean for the next pass); (c) the same tasks under SNF_NO_WINFRONT=1 - the sort path
the front end replaces - give equal calls in every field except cluster_seed_index.  Each case has a host-tier form and a `-m gpu`
form."""
import re

import numpy as np
import pytest

import size_classes as sc
import window_cases as wc
from sniffles_amd import lib
from sniffles_amd.config import SnifflesConfig
from test_size_classes import final, prof, same_as_oracle, use_tier

T = sc.window_thresholds()
W0 = T["w_max_default"]             # the width a batch of small windows gets
CAP, MID, WAVE = T["win_maxcap"], T["win_mid"], sc.WAVE
BIG = 10 << W0                      # bins of a contig long enough for every table that names windows 0 .. 9 of the widest kind


# ---------------------------------------------------------------------------------------------- the literals
def test_window_literals_are_found_and_related():
    assert T["win_maxcap"] == sc.thresholds()["win_maxcap"]
    for k, v in T.items():
        assert isinstance(v, int) and v > 0, k


@pytest.mark.parametrize("name,old,new", [
    ("snf_stage_window.h", "<< 12) | (hap << 13)", "<< 13) | (hap << 14)"),          # written with one literal, read with another
    ("snf_stage_window.h", "#define SNF_WIN_MAXCAP 1024", "#define SNF_WIN_MAXCAP 4096"),   # 63 + 4096 no longer fits the rank field
    ("snf_stage_window.h", "& 31u", "& 15u"),                                        # (63 + 1024) / 64 = 16 no longer fits the block distance
    ("snf_knobs.h", "v <= 12 ? v", "v <= 13 ? v"),                                   # a 13-bit bin
    ("snf_lib.hip", "T < (1 << 17)", "T < (1 << 18)"),                                # t * 8 + svtype beyond 20 bits
    ("snf_lib.hip", "WIN_W_MIN = 6;", "WIN_W_MIN = six;"),                            # a literal no longer found
])
def test_a_broken_window_literal_is_an_error(monkeypatch, name, old, new):
    real = sc._src
    assert old in real(name)
    monkeypatch.setattr(sc, "_src", lambda n: real(n).replace(old, new) if n == name else real(n))
    with pytest.raises(AssertionError):
        sc.window_thresholds()


# ---------------------------------------------------------------------------------------------- the tables
def case(sections, contig_len=BIG * 100, W=W0, cfg=None, env=None, n_tasks=None, bs=100, launches="one launch", expect=None, seed=0):
    return dict(sections=sections, contig_len=contig_len, W=W, cfg=dict(cfg or {}), env=dict(env or {}), n_tasks=n_tasks, bs=bs,
                launches=launches, expect=expect or {}, seed=seed)


def fill_to(pos, have=0, task=0, first=0):
    """Lone INS leads (INS windows come first in the bucket array, one lead seeds nothing) until the next window begins at block
    position `pos`, `have` positions being taken by other windows in front of it already."""
    return wc.lone(task, "INS", (pos - have) % WAVE, W0, first=first)


CASES = {}


def _blocks():
    c = {}
    # a block that owns 64 one-lead windows and seeds nothing (nw = 64), followed by a block of ordinary clusters
    c["blocks_64_lone_windows"] = case([("shuffle", wc.lone(0, "INS", WAVE, W0) + wc.clusters(0, "DEL", 0, W0, [3, 9, 2, 5, 17, 4]))], contig_len=(WAVE + 2 << W0) * 100,
                                       expect=dict(n_valid=WAVE + 40))
    # 62 one-lead windows, a two-lead window on positions 62 - 63, a 65-lead window on position 0 of the next block
    c["blocks_62_lone_a_pair_then_65"] = case([("shuffle", wc.lone(0, "INS", 62, W0) + [(0, "DEL", 5, 2, "plain", "pair"), (0, "DEL", (1 << W0) + 5, WAVE + 1, "plain", "big")] +
                                                wc.clusters(0, "DEL", 3, W0, [4, 6]))], contig_len=(WAVE + 2 << W0) * 100,
                                               expect=dict(start=dict(pair=62, big=WAVE)))
    # the first owned window of a block on its position 1 / 63 (xlo): a window of 65 / 127 leads from position 0 reaches into it
    for n in (WAVE + 1, 2 * WAVE - 1):
        c[f"blocks_first_owned_at_{n - WAVE}"] = case([("shuffle", [(0, "DEL", 5, n, "plain", "big"), (0, "DEL", (2 << W0) + 9, 5, "plain", "next")] + wc.clusters(0, "DUP", 1, W0, [3, 70, 8]))],
                                                      expect=dict(start=dict(big=0, next=n)))
    # 200 leads from position 63: the blocks in its middle own nothing (nw = 0)
    c["blocks_200_from_63"] = case([("shuffle", fill_to(63) + [(0, "DEL", 5, 200, "plain", "big")] + wc.clusters(0, "DEL", 2, W0, [6, 3]) + wc.clusters(0, "INV", 0, W0, [64, 5]))],
                                   contig_len=(WAVE + 2 << W0) * 100, expect=dict(start=dict(big=63)))
    # a window whose last lead lies on position 63, the next on position 0
    c["blocks_window_ends_on_63"] = case([("shuffle", [(0, "DEL", 5, 60, "plain"), (0, "DEL", (1 << W0) + 5, 4, "plain", "last"), (0, "DEL", (2 << W0) + 5, 7, "plain", "next"),
                                                      (0, "DEL", (3 << W0) + 5, WAVE - 7, "plain"), (0, "DEL", (4 << W0) + 5, 130, "plain", "full")])],
                                         expect=dict(start=dict(last=60, next=WAVE, full=2 * WAVE)))
    # n_valid = 64 m - 1 / 64 m / 64 m + 1: the last block partial or exactly full
    for d in (-1, 0, 1):
        n = 3 * WAVE + d
        c[f"blocks_n_valid_{n}"] = case([("shuffle", wc.clusters(0, "DEL", 0, W0, [20, 44, 30, 34]) + [(0, "DUP", 5, WAVE + d, "plain")])], expect=dict(n_valid=n, N=n))
    # more than 64 leads dropped (outside their contig): trailing blocks begin behind n_valid
    L = BIG * 100
    c["blocks_trailing_blocks_behind_n_valid"] = case([("shuffle", wc.clusters(0, "DEL", 0, W0, [20, 43, 7]) + [(0, "DEL", None, 40, "at:-1"), (0, "INS", None, 35, f"at:{L}"), (0, "BND", None, 3, f"at:{L + 1}")])],
                                                     contig_len=L, expect=dict(n_valid=70, N=148))
    # an empty task and a task whose leads are all dropped between two ordinary tasks
    c["blocks_empty_and_dropped_tasks"] = case([("shuffle", wc.clusters(0, "DEL", 0, W0, [5, 9]) + [(2, "DEL", None, 6, "at:-1"), (2, "INS", None, 4, "at:5000")] + wc.clusters(3, "DEL", 0, W0, [8, 3]) +
                                                 wc.clusters(3, "INS", 1, W0, [70]))], contig_len={0: L, 1: 3000, 2: 5000, 3: L}, expect=dict(n_valid=95, N=105))
    return c


def _rounds():
    c = {}
    # windows of 65 ... 130 leads in which a bin of 20 leads covers sorted positions 55 ... 74 (54 ... 73: its 10th / 11th lead on
    # positions 63 / 64) of the block: the head of the bin lies in the round before.  Bins lie in ascending order in the sorted window, so
    # the sizes of the bins in front place a bin exactly; long leads on either side of the border move the three rank carries
    for head, total in ((55, WAVE + 21), (54, 2 * WAVE + 2), (55, 2 * WAVE + 1)):
        front = [25, head - 25 - 8, 8]
        back = [total - head - 20 - 6, 6] if total - head - 20 > 6 else [total - head - 20]
        kinds = ["long4", "hap", "len:2", "ins20"] + ["long4", "len:1"][:len(back)]
        c[f"rounds_bin_of_20_from_{head}_of_{total}"] = case([("shuffle", wc.bins_in_window(0, "INS", 0, W0, front + [20] + back, kinds, name="win") + wc.clusters(0, "DEL", 0, W0, [4, 5]))],
                                                           expect=dict(start=dict(win=0), largest=total))
    # the same around positions 64 k, k = 1 ... 4, in the 256-lead instance: 256 leads from position 63 (positions 63 ... 318)
    sizes = [1, 12, 40, 22, 50, 14, 60, 21, 36]          # bins begin on 63, 64, 76, 116, 138, 188, 202, 262, 283: borders at 64, 128, 192, 256 lie inside bins
    kinds = ["plain", "long4", "hap", "ins20", "len:30", "long", "long4", "ins20", "len:2"]
    c["rounds_256_from_63"] = case([("shuffle", fill_to(63) + wc.bins_in_window(0, "INS", WAVE, W0, sizes, kinds, name="win") + wc.clusters(0, "DEL", 0, W0, [4, 5]))],
                                   contig_len=(WAVE + 2 << W0) * 100, expect=dict(start=dict(win=63), largest=MID))
    # ... and around position 1024 in the largest instance: SNF_WIN_MAXCAP leads from position 63 (j reaches 16).  One bin of more than
    # 256 leads keeps every width above 256, so the widest width is kept
    for total in (CAP - 1, CAP):
        sizes = [MID + 44, 300, 350, 6, 20, 30, total - (MID + 44) - 300 - 350 - 6 - 20 - 30]      # bins begin on 63, 363, 663, 1013, 1019, 1039, 1069
        kinds = ["plain", "plain", "plain", "plain", "plain", "plain", "plain"]
        c[f"rounds_{total}_from_63"] = case([("shuffle", wc.lone(0, "DEL", 63, W0) + wc.bins_in_window(0, "DEL", 63, W0, sizes, kinds, name="win") + wc.clusters(0, "DUP", 0, W0, [4, 5]))],
                                            contig_len=(WAVE + 2 << W0) * 100, expect=dict(start=dict(win=63), largest=total))
    sizes = [MID + 44, 300, 340, 12, 24, 30, CAP - (MID + 44) - 300 - 340 - 12 - 24 - 30]
    kinds = ["long4", "hap", "len:200", "long4", "ins20", "long", "len:2"]      # INS: seeds, `leads` and `leads_long` on both sides of position 1024
    c["rounds_1024_ins_from_63"] = case([("shuffle", fill_to(63) + wc.bins_in_window(0, "INS", WAVE, W0, sizes, kinds, name="win") + wc.clusters(0, "DEL", 0, W0, [4, 5]))],
                                        contig_len=(WAVE + 2 << W0) * 100, expect=dict(start=dict(win=63), largest=CAP))
    return c


def _bins():
    c = {}
    for name, cfg in (("default", {}), ("max_reads_bin_1", dict(consensus_max_reads_bin=1)), ("max_reads_bin_2000", dict(consensus_max_reads_bin=2000)),
                      ("mosaic", dict(mosaic=True)), ("min_leads_3", dict(dev_min_leads_cluster=3)), ("min_leads_3_mosaic", dict(dev_min_leads_cluster=3, mosaic=True))):
        c["bins_" + name] = case(wc.bins_sections(), contig_len=wc.TABLE_BINS * 100, cfg=cfg, seed=3)
    return c


def _borders():
    c = {}
    for W, env in ((6, dict(SNF_WIN_BITS="6")), (8, dict(SNF_WIN_BITS="8")), (10, dict(SNF_WIN_BITS="10")), (12, dict(SNF_WIN_BITS_MAX="12", SNF_WIN_BITS="12"))):
        for d in (-1, 0, 1):
            L = 100 * (1 << W) * 3 + d
            c[f"borders_W{W}_contig_{'3_windows' + ('%+d' % d if d else '')}"] = case(wc.borders_sections(W, L), contig_len=L, W=W, env=env)
    # a contig shorter than one bin; cluster_binsize 25 and 200
    c["borders_contig_shorter_than_a_bin"] = case([("shuffle", [(0, "DEL", 0, 4, "plain"), (0, "DEL", None, 2, "at:60"), (0, "DEL", None, 2, "at:-1")] + wc.clusters(1, "DEL", 0, W0, [5, 3]))],
                                                  contig_len={0: 60, 1: BIG * 100}, expect=dict(n_valid=12))
    for bs in (25, 200):
        for d in (-1, 0, 1):
            L = bs * (1 << W0) * 2 + d
            c[f"borders_binsize_{bs}_contig{d:+d}"] = case(wc.borders_sections(W0, L, bs), contig_len=L, bs=bs, cfg=dict(cluster_binsize=bs))
    return c


def two_bins(a, b, apart=512):
    return [("shuffle", [(0, "DEL", 2048, a, "plain"), (0, "DEL", 2048 + apart, b, "plain")] + wc.clusters(0, "INS", 0, W0, [5, 3]))]


def relayout_sections(b):
    return [("shuffle", [(0, "DEL", 2048, 300, "plain"), (0, "DEL", 2304, b, "plain"), (0, "DEL", 2560, 400, "plain")] + wc.clusters(0, "INS", 0, W0, [5, 3]))]


def _widths():
    c = {}
    # 256 leads in one window of the widest kind: it stays; 128 + 129 leads in bins 512 apart: one width down
    for a, b, W in ((MID // 2, MID // 2 - 1, W0), (MID // 2, MID // 2, W0), (MID // 2, MID // 2 + 1, W0 - 1)):
        c[f"width_{a}+{b}"] = case(two_bins(a, b), W=W, expect=dict(largest=a + b if W == W0 else max(a, b)))
    # 300 + 400 + 400: no width gives 256, the first that gives SNF_WIN_MAXCAP is taken after the loop has reached WIN_W_MIN (the
    # re-layout branch); 300 + 724 is the most that width holds, 300 + 725 goes one further down
    for b, W in ((400, W0 - 1), (CAP - 300, W0 - 1), (CAP - 300 + 1, W0 - 2)):
        c[f"width_relayout_300+{b}+400"] = case(relayout_sections(b), W=W, expect=dict(largest=300 + b if W == W0 - 1 else max(b, 400)))
    # more than SNF_WIN_MAXCAP leads in one bin: off
    c["width_1025_in_one_bin_off"] = case([("shuffle", [(0, "DEL", 2048, CAP + 1, "plain")] + wc.clusters(0, "INS", 0, W0, [5, 3]))], W=None)
    # SNF_WIN_BITS = 5 and = SNF_WIN_BITS_MAX + 1 behave as unset
    for bits in (T["w_min"] - 1, W0 + 1):
        c[f"width_forced_{bits}_is_as_unset"] = case(two_bins(MID // 2, MID // 2 + 1), W=W0 - 1, env=dict(SNF_WIN_BITS=str(bits)))
    return c


def split_sections(n_leads, big, big_size):
    """`big` windows of `big_size` leads, each beginning in a block of its own, one of exactly 64, and small clusters up to n_leads leads in all."""
    es = []
    for k in range(big):
        es += [(0, "DEL", (k << W0) + 5, big_size, "plain"), (0, "DEL", (k << W0) + 45, (-big_size) % WAVE + 2 * WAVE, "hap")]
    es.append((0, "DUP", 5, WAVE, "plain"))          # a window of exactly 64 leads stays with the small instance
    used = sum(e[3] for e in es)
    rest = n_leads - used
    assert rest >= 0
    k = 0
    while rest > 0:
        n = min(rest, 3 + k % 5)
        es.append((0, "INS", ((k // 12) << W0) + 7 + 30 * (k % 12), n, "long4" if k % 3 == 0 else "plain"))      # (twelve bins a window: at most 57 leads)
        rest -= n
        k += 1
    return [("shuffle", es)]


def _split():
    c = {}
    env = dict(SNF_W4_SPLIT="1")
    # one window above 64 leads: n_blk = 8 -> one launch, 9 -> two
    for n, launches in ((8 * WAVE, "one launch"), (8 * WAVE + 1, "two launches")):
        c[f"split_one_big_window_{n}_leads"] = case(split_sections(n, 1, 300), contig_len=(WAVE + 2 << W0) * 100, env=env, launches=launches, expect=dict(N=n, largest=300 + 148))
    # four of them, each beginning in a block of its own (the list is as long as the second grid); both large instances
    c["split_four_big_windows_256"] = case(split_sections(33 * WAVE, 4, 100), contig_len=(WAVE + 2 << W0) * 100, env=env, launches="two launches", expect=dict(big64=4, largest=MID))
    c["split_four_big_windows_1024"] = case(split_sections(33 * WAVE, 4, 300), contig_len=(WAVE + 2 << W0) * 100, env=env, launches="two launches", expect=dict(big64=4, largest=300 + 148))
    return c


def _groups():
    """win_group (w1_hist / w3_scatter): the lanes of a wave that hit one window share an atomic."""
    c = {}
    for n in (MID - 1, MID, MID + 1):          # N = 255 / 256 / 257: the last workgroup of w1 / w3 full, one lead short, one lead alone
        secs = [("plan", [(0, "DEL", 5, WAVE, "plain")]),                                              # 64 consecutive input leads in one window
                ("plan", wc.lone(0, "DUP", WAVE, W0)),                                                 # the 64 of the next wave in 64 windows
                ("robin", [(0, "INV", 5, 24, "plain"), (0, "INV", (3 << W0) + 5, 24, "plain")]),        # alternating between two windows
                ("robin", [(0, "INS", 5, 16, "long4"), (0, "INS", 45, 16, "plain"), (0, "INS", None, 16, "at:-1")])]      # every third lead dropped
        have = sum(e[3] for _, es in secs for e in es)
        secs.append(("plan", [(0, "BND", (k << W0) + 5, 1, "plain") for k in range(n - have - 2)] + [(0, "DEL", 45, 2, "plain")]))      # consecutive leads in windows of their own
        c[f"groups_{n}_leads"] = case(secs, contig_len=(WAVE + 2 << W0) * 100, expect=dict(N=n, n_valid=n - 16))
    return c


def tiles_sections(n_tasks, n_leads, gap=30):
    es = []
    for t in range(n_tasks):
        es += [(t, "INS", 5, 3, "plain"), (t, "DEL", 5, 4, "plain"), (t, "DUP", 5, 2, "plain"), (t, "INV", 5, 2, "plain"), (t, "BND", 5, 2, "plain")]
    rest = n_leads - sum(e[3] for e in es)
    k = 0
    while rest > 0:          # cheap DEL leads: clusters of 40 in the last task, `gap` bins apart
        n = min(rest, 40)
        es.append((n_tasks - 1, "DEL", 35 + gap * k, n, "plain"))
        rest -= n
        k += 1
    return [("shuffle", es)]


def _tiles():
    """The scans of w2 (over the window slots) and w5 (over the blocks) work in tiles of 256.  A task has 7 window slots per window of
    its contig, so the slots of a batch come in sevens: 252 / 259 and 511 / 518 are the nearest to a tile's end, with occupied windows
    on the last slot of a tile and the first of the next (slots 255 / 256: the INV and BND windows of the 37th task; 511 / 512: the INS
    and DEL windows of the 74th).  n_blk = 256 / 257 takes 16 384 / 16 385 leads: DEL clusters of 40, at most five in a window."""
    c = {}
    for slots in (252, 259, 511, 518):
        for chain in "01":
            nt = slots // 7
            c[f"tiles_{slots}_slots_chain{chain}"] = case(tiles_sections(nt, 13 * nt + 90), contig_len=90_000, n_tasks=nt, env=dict(SNF_CHAIN=chain), expect=dict(NW=slots))
    for blk in (MID, MID + 1):
        for chain in "01":
            n = WAVE * blk if blk == MID else WAVE * MID + 1
            c[f"tiles_{blk}_blocks_chain{chain}"] = case(tiles_sections(2, n, gap=205), contig_len=(90 << W0) * 100, env=dict(SNF_CHAIN=chain), expect=dict(N=n))
    return c


def _tables():
    """The tables with fixtures from the unmodified reference (tests/cases.py: window_edges_*), as the handle lays them out."""
    return dict(table_blocks_rounds=case(wc.blocks_rounds_sections(), contig_len=wc.TABLE_BINS * 100, seed=11,
                                         expect=dict(start=dict(pair=62, mid=WAVE, two_rounds=5 * WAVE + 1, ends_on_63=451, on_0=9 * WAVE), largest=MID, big64=4, N=651)),
                table_borders=case(wc.borders_sections(wc.TABLE_W, wc.TABLE_BORDERS_LEN), contig_len=wc.TABLE_BORDERS_LEN, seed=5, expect=dict(N=33, n_valid=27)))


for _f in (_blocks, _rounds, _bins, _borders, _widths, _split, _groups, _tiles, _tables):
    CASES.update(_f())


# ---------------------------------------------------------------------------------------------- the check
def equal_but_seed_index(a, b):
    assert len(a.calls) == len(b.calls) and np.array_equal(a.task_call_off, b.task_call_off)
    for f in a.calls.dtype.names:
        if f != "cluster_seed_index":
            assert np.array_equal(a.calls[f], b.calls[f], equal_nan=a.calls[f].dtype.kind == "f"), f


def check_case(tier, name, oracle_mod, monkeypatch, capfd, passes=2):
    c = CASES[name]
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    tis = wc.build(c["sections"], c["contig_len"], c["n_tasks"], c["bs"], c["seed"])
    geo = (c["sections"], c["contig_len"], c["n_tasks"], c["bs"])
    forced, w_max = int(c["env"].get("SNF_WIN_BITS", 0)), int(c["env"]["SNF_WIN_BITS_MAX"]) if "SNF_WIN_BITS_MAX" in c["env"] else None
    assert wc.chosen_width(*geo, w_max=w_max, forced=forced) == c["W"]              # the plan against the rule as read from the sources
    info = wc.layout(c["sections"], c["W"] if c["W"] is not None else W0, c["contig_len"], c["n_tasks"], c["bs"])
    for k, v in c["expect"].items():                                              # ... and against the numbers the case was written for
        if k == "start":
            for nm, pos in v.items():
                assert info["start"][nm] == pos, (nm, info["start"])
        else:
            assert info[k] == v, (k, info[k], v)
    assert info["N"] == sum(ti.n_leads for ti in tis)
    cfg = SnifflesConfig(**c["cfg"])
    exp = oracle_mod.run(cfg, tis, True)
    capfd.readouterr()
    with lib.Batch(cfg, tis) as b:
        lines = prof(capfd)["window front end"]
        assert len(lines) == 1, lines
        if c["W"] is None:
            assert "window front end: off " in lines[0], lines
        else:
            assert wc.profile_text(info, c["launches"]) in lines[0], (lines, wc.profile_text(info, c["launches"]))      # (a)
        for _ in range(passes):                                                                                          # (b)
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
        b.call_candidates(); b.finalize()
        got = b.fetch(1)
        same_as_oracle(got, exp, tis)
    monkeypatch.setenv("SNF_NO_WINFRONT", "1")                                                                           # (c)
    capfd.readouterr()
    with lib.Batch(cfg, tis) as b:
        assert prof(capfd)["window front end"] == []
        b.call_candidates(); b.finalize()
        equal_but_seed_index(got, b.fetch(1))
    return exp, tis


NAMES = sorted(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_window_front_end_host(name, oracle_mod, monkeypatch, capfd):
    check_case("host", name, oracle_mod, monkeypatch, capfd, passes=3 if name.startswith("split_") else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_window_front_end_gpu(name, oracle_mod, monkeypatch, capfd):
    check_case("gpu", name, oracle_mod, monkeypatch, capfd, passes=3 if name.startswith("split_") else 2)


@pytest.mark.parametrize("name,case_name", [("window_edges_blocks_rounds", "table_blocks_rounds"), ("window_edges_bins", "bins_default"),
                                            ("window_edges_bins_mosaic", "bins_mosaic"), ("window_edges_borders", "table_borders")])
def test_window_fixtures_are_the_tables_checked_here(name, case_name):
    """The registered cases (tests/cases.py) are the tables whose layouts the tests above assert, with the options they run under, and
    the fixtures were recorded from exactly these inputs."""
    import cases
    import golden_util as gu
    build, kw, _ = cases.ALL[name]
    c = CASES[case_name]
    ti = build()
    assert gu.input_sha(ti) == gu.input_sha(wc.build(c["sections"], c["contig_len"], c["n_tasks"], c["bs"], c["seed"])[0]) == gu.load(name)["input_sha"]
    assert kw == c["cfg"] and c["W"] == wc.TABLE_W == W0 and not c["env"]
    assert len(gu.load(name)["expected"]["final"]) >= 4      # (the borders table: the two bin pairs, bin 0, the contig's last bin)


def test_the_sequence_cap_changes_the_consensus_of_the_bins_table(oracle_mod):
    """The INS alleles of the `ins20` bins are mutated enough that a vote without the 11th and 12th lead's sequences gives another
    string: with consensus_max_reads_bin = 10 (default) the oracle's ALTs differ from those with 2000, and with 1 from both - so a
    front end that drops the wrong lead's sequence, or none, cannot give the oracle's records."""
    tis = [wc.table_bins()]
    alts = {}
    for cap in (1, 10, 2000):
        res = oracle_mod.run(SnifflesConfig(consensus_max_reads_bin=cap), tis, True)
        alts[cap] = [r.get("alt") for r in final(res, tis)[0] if r["svtype"] == "INS"]
        assert len(alts[cap]) >= 12
    assert alts[10] != alts[2000] and alts[1] != alts[10] and alts[1] != alts[2000]


# ---------------------------------------------------------------------------------------------- the width switch out of range
def knob_sections():
    """70 two-lead DEL clusters in bins 1024 k + 3: with 13-bit windows bin 4096 + 3 of a window would need the 13th bit of win_pack's
    bin field, where is_long lives."""
    return [("shuffle", [(0, "DEL", 1024 * k + 3, 2, "plain") for k in range(70)])]


def check_width_switch_out_of_range(tier, value, oracle_mod, monkeypatch, capfd):
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    monkeypatch.setenv("SNF_WIN_BITS_MAX", value)
    L = 100 * 1024 * 71
    tis = wc.build(knob_sections(), L)
    cfg = SnifflesConfig()
    exp = oracle_mod.run(cfg, tis, True)
    assert len(exp.calls) == 70
    info = wc.layout(knob_sections(), W0, L)       # out of range is as unset: the default width
    capfd.readouterr()
    with lib.Batch(cfg, tis) as b:
        lines = prof(capfd)["window front end"]
        assert len(lines) == 1 and int(re.search(r"W = (\d+):", lines[0]).group(1)) <= T["w_max_hi"], lines
        assert wc.profile_text(info) in lines[0], lines
        for _ in range(2):
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
        b.call_candidates(); b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)


@pytest.mark.parametrize("value", ["13", "5"])
def test_width_switch_out_of_range_is_as_unset_host(value, oracle_mod, monkeypatch, capfd):
    check_width_switch_out_of_range("host", value, oracle_mod, monkeypatch, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["13", "5"])
def test_width_switch_out_of_range_is_as_unset_gpu(value, oracle_mod, monkeypatch, capfd):
    check_width_switch_out_of_range("gpu", value, oracle_mod, monkeypatch, capfd)
