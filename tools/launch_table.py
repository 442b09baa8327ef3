"""
Record tests/golden/launch_table.json (tests/launch_table.py says what is in it).

Run on the GPU, on a checkout of the commit whose behaviour is to be kept -- the parent of a host-layer refactor, never
the refactored branch itself:

    python tools/launch_table.py OUT.json [EARLIER.json]

With EARLIER.json (a first recording of the same commit) every output hash that differs between the two recordings is
left out (null) and named on stdout: such an application is not reproducible bit for bit, and the tolerance tests cover
it.  Anything else that differs between the two recordings is an error.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import sdfs_via_autodiff_amd as S
    import launch_table as LT
    out = sys.argv[1]
    rec = LT.record_all(S)
    nhash = sum(len(c["hashes"]) for c in rec["applications"].values())
    dropped = []
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            old = json.load(f)
        for name, c in rec["applications"].items():
            for k, hx in c["hashes"].items():
                if old["applications"][name]["hashes"][k] != hx:
                    c["hashes"][k] = old["applications"][name]["hashes"][k] = None
                    dropped.append(f"{name}: {k}")
        if old != rec:
            for part in ("applications", "loops"):
                for name in rec[part]:
                    if old[part].get(name) != rec[part][name]:
                        print("DIFFERS", name, old[part].get(name), rec[part][name])
            sys.exit("the two recordings differ in more than output hashes")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['applications'])} application cases, {nhash} output hashes, {len(rec['loops'])} loop cases -> {out}")
    for d in dropped:
        print("not reproducible, hash left out:", d)


if __name__ == "__main__":
    main()
