"""
Record tests/golden/analysis_table.json (tests/analysis_table.py says what is in it).

Run on the GPU, on a checkout of the commit whose behaviour is to be kept -- the parent of a refactor of the analysis
layer, never the refactored branch itself:

    python tools/analysis_table.py OUT.json [EARLIER.json]

With EARLIER.json (a first recording of the same commit) every output hash that differs between the two recordings is
left out (null) and named on stdout: such an output is not reproducible bit for bit, and the tolerance tests cover it.
Anything else that differs between the two recordings is an error.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import sdfs_via_autodiff_amd as S
    import analysis_table as AT
    out = sys.argv[1]
    rec = AT.record_all(S)
    calls = [(name, call, c) for name, case in rec.items() for call, c in case.items()]
    dropped = []
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            old = json.load(f)
        for name, call, c in calls:
            for k, hx in c["hashes"].items():
                if old[name][call]["hashes"][k] != hx:
                    c["hashes"][k] = old[name][call]["hashes"][k] = None
                    dropped.append(f"{name}: {call}: {k}")
        if old != rec:
            for name, call, c in calls:
                if old[name].get(call) != c:
                    print("DIFFERS", name, call, old[name].get(call), c)
            sys.exit("the two recordings differ in more than output hashes")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases, {len(calls)} calls, {sum(len(c['hashes']) for _, _, c in calls)} output hashes -> {out}")
    for d in dropped:
        print("not reproducible, hash left out:", d)


if __name__ == "__main__":
    main()
