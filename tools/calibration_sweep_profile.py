#!/usr/bin/env python3
"""
Build profiles/calibration_sweep_errors.txt from the figures tests/test_hip_calibrations.py prints.

    python -m pytest tests/test_hip_calibrations.py -q -m gpu -s > sweep.log
    python tools/calibration_sweep_profile.py sweep.log "<machine>" <commit> profiles/calibration_sweep_errors.txt

Lines read:  CALSWEEP <family> <calibration> <quantity ...> <measured> <bound>     (the tests' note())
             F32-MEASURED ssy (<shape>) calibration <name> ... mode <k>: <C>      (tests/test_hip_f32_forms.py report())
One row per (family, calibration, quantity): the largest measured value beside its bound.  Quantities that the tests
print once per level of w, per parameter or per SA length are folded into one row (the maximum).
"""
import collections
import re
import sys

MEMBERS = ["0 member(0)", "1 member(1)", "2 steep", "3 shallow", "4 positive", "5 fractional", "6 linear", "7 shifted"]
HEADER = """Worst measured error of every quantity of tests/test_hip_calibrations.py beside its bound, per calibration and family
(the maximum over the two levels of w, over the parameters, or over the three SA lengths, where a row says so).
Machine: {machine}; library built from commit {commit} (the tests change no library code).
Made by tools/calibration_sweep_profile.py from the CALSWEEP / F32-MEASURED lines of
python -m pytest tests/test_hip_calibrations.py -q -m gpu -s.
For the fp32 forms the figure is the fraction of the derived bound used (tests/f32_bound.py): err / (C u (J|v| + m|v|))
over m = 0, 1 for krylov_f32, max err / t32_bound(T, theta) for t_f32.
Padded families: pad16 = GCY 10^6 (16-wide tiles), pad20 = SSY 20^4 (20), pad32 = SSY (25,18,32,7) (32 and 32),
pad24_32 = SSY (22,18,32,7) (32 and 24); each case asserts these widths from describe_plan().
Full-range rows: the relative error of the finite entries of T w after each value is added (stages without a finite
entry -- all +inf or all NaN -- are compared exactly and have no row).
Not in the table because they are exact: index paths equal to the numpy twin bit for bit; status 0 for every batch
member; the reversed batch equal to the reversed result bit for bit; NaN and +inf patterns of the full-range cases.
"""


def main(log_path, machine, commit, out_path):
    rows = collections.OrderedDict()                 # (part, family, calibration, quantity) -> (worst, bound)

    def put(part, fam, cal, q, e, b):
        k = (part, fam, cal, q)
        if k not in rows or e > rows[k][0]:
            rows[k] = (e, b)

    for ln in open(log_path, errors="replace").read().splitlines():
        i = ln.find("CALSWEEP ")
        if i >= 0:
            t = ln[i:].split()
            fam, cal, e, b = t[1], t[2], float(t[-2]), float(t[-1])
            q = re.sub(r" L(600|5)$", "", " ".join(t[3:-2]))
            if q.startswith("tangent "):
                part, name = "4 parameter tangents", q.split()[1]
                same = [k for k in rows if k[:3] == (part, fam, cal)]
                if same and rows[same[0]][0] >= e:
                    continue
                for k in same:
                    del rows[k]
                q = f"dT/dp, worst parameter ({name})"
            elif fam.startswith("batch-"):
                part = "4 batch kernels"
                cal = MEMBERS[int(cal[6:])] if cal.startswith("member") else "all members"
                q = re.sub(r"^gradient .*", "gradient, worst parameter", q)
                q = re.sub(r"^SA k=\d", "SA k = 1, 2, 3", q)
            elif fam.startswith("t_f32-"):
                part, fam = "3 t_f32", fam[6:]
            elif fam == "simulate":
                part = "4 simulate (SSY 5x4x6x7)"
            elif q == "tilted product":
                part = "4 tilted products (SSY 15^4)"
            elif q.startswith("full range"):
                part = "2 full-range power path"
            else:
                part = "2 operator"
            put(part, fam, cal, q, e, b)
        m = re.search(r"F32-MEASURED ssy \(([\d, ]+)\) calibration (\w+) .* mode (\d): ([\d.]+)", ln)
        if m:
            shp = tuple(int(x) for x in m.group(1).split(","))
            mode, c = int(m.group(3)), float(m.group(4))
            C = 8 + (sum(shp) if shp == (16, 16, 24, 24) and mode == 3 else 0)      # (the fp32-MFMA kernels ran)
            put("3 krylov_f32", "ssy" + "x".join(map(str, shp)), m.group(2), f"mode {mode} (C = {C})", c / C, 1.0)

    out = [HEADER.format(machine=machine, commit=commit)]
    part = None
    for (p, fam, cal, q), (e, b) in sorted(rows.items()):
        if p != part:
            part = p
            out += ["", "== part " + p + " ==",
                    f"{'family':<16} {'calibration':<13} {'quantity':<46} {'worst':>10} {'bound':>9} {'worst/bound':>11}"]
        out.append(f"{fam:<16} {cal:<13} {q:<46} {e:>10.3e} {b:>9.1e} {e / b:>11.2e}")
    open(out_path, "w").write("\n".join(out) + "\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main(*sys.argv[1:5])
