"""Records tests/golden/launch_sequence.json: the (name, bytes) of every bracketed operation of a pass, per tier, form and pass, from
the library as it is built now (tests/launch_sequence_cases.py holds the batch, the forms and the passes; tests/test_launch_sequence.py
compares against the file).  Record it from the commit whose sequence is to be kept, BEFORE changing the library.

  python tools/record_launch_sequence.py host          the host tier (tests/emu) - no device needed
  python tools/record_launch_sequence.py gpu           the real library on device 0
  python tools/record_launch_sequence.py host gpu [-o FILE]

A tier that is not named keeps what the file holds for it; a tier whose lists equal the other's is stored as that tier's name."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import launch_sequence_cases as C  # noqa: E402
from sniffles_amd import lib, records  # noqa: E402


def record_tier(tier):
    if tier == "host":
        import emu.emu as E
        E.lib()
    else:
        import torch
        torch.cuda.init()
        lib.use_library(None)
        assert lib.device_count() >= 1, "no HIP device"
    tis, cfg, exp = C.batch()
    tis = list(tis)
    want = records.records(exp, tis, "final")

    def check(got):
        assert records.records(got, tis, "final") == want, "the pass differs from the oracle: nothing recorded"
    out = {}
    for form in C.FORMS:
        env, gone = C.environment(form)
        saved = {k: os.environ.get(k) for k in list(env) + gone}
        for k in gone:
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            with lib.Batch(cfg, tis) as b:
                out[form] = C.record(b, check)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return out


def dumps(data):
    """One line per pass, so that a change of the sequence reads as a change of lines."""
    tiers = []
    for t in sorted(data):
        if isinstance(data[t], str):
            tiers.append(f' "{t}": {json.dumps(data[t])}')
            continue
        forms = []
        for form in C.FORMS:
            rows = ",\n".join(f'   "{p}": {json.dumps(data[t][form][p], separators=(",", ":"))}' for p in C.PASSES)
            forms.append(f'  "{form}": {{\n{rows}\n  }}')
        tiers.append(f' "{t}": {{\n' + ",\n".join(forms) + "\n }")
    return "{\n" + ",\n".join(tiers) + "\n}\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tiers", nargs="+", choices=C.TIERS)
    ap.add_argument("-o", "--out", default=C.FIXTURE)
    a = ap.parse_args()
    data = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            data = json.load(f)
    for t in C.TIERS:                                # stored names back to lists
        if isinstance(data.get(t), str):
            data[t] = data[data[t]]
    for t in a.tiers:
        data[t] = record_tier(t)
    if all(t in data for t in C.TIERS) and data["gpu"] == data["host"]:
        data["gpu"] = "host"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(dumps(data))
    for t in a.tiers:
        lists = data[t] if not isinstance(data[t], str) else data[data[t]]
        print(t, {form: [len(lists[form][p]) for p in C.PASSES] for form in C.FORMS}, "(same as host)" if data[t] == "host" else "")


if __name__ == "__main__":
    main()
