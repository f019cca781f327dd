"""The cases of tests/test_launch_sequence.py and of tools/record_launch_sequence.py: one batch, the forms of the pass, and how the
(name, bytes) list of every bracketed operation of a pass is taken from a handle.  tests/golden/launch_sequence.json holds the lists
the library gave when the fixture was recorded; the recorder and the test share everything here, so they cannot drift apart."""
import functools
import json
import os

from sniffles_amd import synth
from sniffles_amd.config import SnifflesConfig

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequence.json")
TIERS = ("host", "gpu")
FORMS = {
    "default": {},
    "chain0_graph0": {"SNF_CHAIN": "0", "SNF_GRAPH": "0"},
    "no_winfront": {"SNF_NO_WINFRONT": "1"},
    "no_fuse": {"SNF_NO_FUSE": "1"},
    "no_wave": {"SNF_NO_WAVE": "1"},
}
PASSES = ("first_pass", "second_pass", "candidates_then_finalize")
# every switch that selects a form of the pass or of its timing: a recording starts from none of them
CLEARED = ("SNF_CHAIN", "SNF_NO_CHAIN", "SNF_GRAPH", "SNF_NO_GRAPH", "SNF_NO_WINFRONT", "SNF_NO_FUSE", "SNF_NO_WAVE", "SNF_NO_TIMING",
           "SNF_TIMELINE", "SNF_TIME_EVERY", "SNF_SERIAL", "SNF_READPREP_EACH_PASS", "SNF_D4", "SNF_W4_SPLIT", "SNF_D2_MID",
           "SNF_STAGE_OUT", "SNF_STAGE_COPY", "SNF_CONS_ORDER", "SNF_CONS_NW", "SNF_CONS_LARGE_NW", "SNF_FUSE_COPY")
# what the batch has to reach for the pin to cover the pass: clusters of more than 64 leads in all three stages, both consensus classes
# and the verbatim copies, the window front end, both size classes of refine and call; and, in the form whose passes are eager by the
# library's own rule (a batch this small replays a graph otherwise, and copies in place), the fused-sequence copy on the side stream
REACHED_BY_DEFAULT = {"x_big_refine", "x_big_call", "x_big_finalize", "e45w_consensus_small", "e45w_consensus_large", "e4c_copy",
                      "front_window", "w4s_segment", "d1g_refine8", "d1w_refine", "d2g_call8", "d2w_call", "e1w_finalize"}
REACHED_BY_EAGER = REACHED_BY_DEFAULT | {"d1c_fusecopy"}


@functools.lru_cache(maxsize=None)
def batch():
    """The four tasks of tests/test_knobs.py, the configuration and the oracle's result: computed once, changed by nobody."""
    import oracle
    tis = tuple(synth.gen_fuzz(4242 + k, task_id=k) for k in range(3)) + (synth.gen_task(3, "chrS", 150_000, 40.0, seed=5),)
    cfg = SnifflesConfig()
    return tis, cfg, oracle.run(cfg, list(tis), True)


def environment(form):
    """(to set, to remove) for one form."""
    env = dict(FORMS[form], SNF_TIME_ALL="1")
    return env, [k for k in CLEARED if k not in env]


def sequence(b):
    return [[name, nbytes] for name, _, nbytes in b.timings()]


def record(b, check):
    """The three passes of a form on an open handle; check(result) after each.  Returns {pass: [[name, bytes], ...]}."""
    b.timing_every(1)
    out = {}
    for name in PASSES[:2]:                      # the first is the pass without the handle's histogram
        b.run_pass()
        check(b.fetch(1))
        out[name] = sequence(b)
    b.call_candidates()
    b.finalize()
    check(b.fetch(1))
    out[PASSES[2]] = sequence(b)
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def expected(fixture, tier, form):
    """One copy is kept where the tiers gave the same lists: a tier's entry may be the name of the tier that holds them."""
    lists = fixture[tier]
    return (fixture[lists] if isinstance(lists, str) else lists)[form]
