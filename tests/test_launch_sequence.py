"""The operations a pass enqueues, pinned: under SNF_TIME_ALL every launch, scan, sort and timed copy of a pass is bracketed, and
Batch.timings() lists them in the order they were enqueued, by timing name and algorithmic bytes.  tests/golden/launch_sequence.json
holds those lists per tier, form and pass as the library gave them when it was recorded (tools/record_launch_sequence.py; the batch,
the forms and the passes are tests/launch_sequence_cases.py, shared with the recorder).

What can go wrong when the launch code of snf_lib.hip is rewritten: a launch dropped, doubled or moved; a timing name or a byte count
changed (bench.py, the roofline legs and the committed profiles key on them); a bracket that was "only under SNF_TIME_ALL" becoming
"every sampled pass" or the reverse, which this sees as the same list but tests/test_timing.py sees without the switch.  SNF_TIME_ALL
keeps a pass out of the graph, so this is the eager sequence; the graph tests cover the replayed pass."""
import pytest

import launch_sequence_cases as C
from sniffles_amd import lib
from test_size_classes import same_as_oracle, use_tier

TIERS = [pytest.param("host", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


def test_the_fixture_has_every_case_and_the_batch_reaches_every_class():
    fx = C.load()
    for tier in C.TIERS:
        for form in C.FORMS:
            passes = C.expected(fx, tier, form)
            assert set(passes) == set(C.PASSES), (tier, form)
            for p in C.PASSES:
                assert len(passes[p]) > 20 and all(isinstance(n, str) and isinstance(nb, int) for n, nb in passes[p]), (tier, form, p)
        for form, reached in (("default", C.REACHED_BY_DEFAULT), ("chain0_graph0", C.REACHED_BY_EAGER)):
            for p in C.PASSES:
                names = {n for n, _ in C.expected(fx, tier, form)[p]}
                assert reached <= names, (tier, form, p, sorted(reached - names))
        # the other forms are other forms: the sort path, the rocPRIM scans, the thread-per-item kernels
        names = lambda form: {n for n, _ in C.expected(fx, tier, form)["second_pass"]}
        assert "sort_lead_keys" in names("no_winfront") and "front_window" not in names("no_winfront")
        assert {"scan_bins", "scan_clusters", "sort_lead_keys"} <= names("no_fuse")
        assert {"d1_refine", "d2_call"} <= names("no_wave") and not {"d1w_refine", "d2w_call"} & names("no_wave")
        assert {"w5a_sums", "w5b_offsets"} <= names("chain0_graph0") and "w5c_offsets" in names("default")


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", list(C.FORMS))
def test_a_pass_enqueues_the_recorded_sequence(form, tier, oracle_mod, monkeypatch):
    use_tier(tier, monkeypatch)
    env, gone = C.environment(form)
    for k in gone:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tis, cfg, exp = C.batch()
    tis = list(tis)
    want = C.expected(C.load(), tier, form)
    with lib.Batch(cfg, tis) as b:
        got = C.record(b, lambda res: same_as_oracle(res, exp, tis))
    for p in C.PASSES:
        if got[p] != want[p]:                             # the first difference, readably
            k = next((i for i, (g, w) in enumerate(zip(got[p], want[p])) if g != w), min(len(got[p]), len(want[p])))
            pytest.fail(f"{form} / {p}: operation {k} is {got[p][k:k + 3]}, recorded {want[p][k:k + 3]} "
                        f"({len(got[p])} operations, recorded {len(want[p])})")
