#!/usr/bin/env python3
"""tools/twoval_mutations.py -- do the cases of tests/twoval_cases.py discriminate?  Applies one small mutation at a time to a temporary copy of
csrc/amwg_twoval.h, builds tests/host/twoval_eval_host.cpp against the copy FOR THE HOST (nothing is written into the tree, nothing runs on a GPU) and counts the
lanes whose sum differs from the plain sequential sum, by lane range and census class.  Prints the table of tests/README.twoval.md.  Exit status 1 if a mutation
that is not listed as equivalent survives, or if one listed as equivalent is caught.      python tools/twoval_mutations.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import twoval_cases as V      # noqa: E402
from test_twoval_host import build_host      # noqa: E402

ROUND = "(r > h ? 1u : 0u)"
MUTATIONS = [      # (name, old, new, occurrences of old in the header -- all are replaced --, equivalent: README.twoval.md has the argument)
    ("tie rounds up: r > h -> r >= h (equivalent)", ROUND, "(r >= h ? 1u : 0u)", 2, True),
    ("limit larger by one", "const uint64_t limit = (1ull << 53) - A;", "const uint64_t limit = (1ull << 53) - A + 1;", 1, False),
    ("stall exit ignores the tie", "if (mulA == 0 && mulB == 0 && mode == 0) break;", "if (mulA == 0 && mulB == 0) break;", 1, False),
    ("saturation of n * mul removed (hi << 32 wraps)", "if (hi >> 21) return kSat;", "", 1, False),
    ("hi >> 21 -> hi >> 22 (equivalent)", "if (hi >> 21) return kSat;", "if (hi >> 22) return kSat;", 1, True),
    ("s >= 54 -> s >= 53", "if (s >= 54) {", "if (s >= 53) {", 2, False),
    ("e >= emax + 1 -> e >= emax (equivalent)", "if (!(e >= emax + 1 && e < 0x7ff))", "if (!(e >= emax && e < 0x7ff))", 1, True),
    ("mode 1: first-addition correction dropped", "if (m > i) { const uint64_t qf = bit_i ? q1 : q0; T = T - (qf + (qf & 1ull)) + qf + ((p + qf) & 1ull); }", "", 1, False),
    ("mode 2: first tie rounded by qt & 1", "if (nt) T += ((p + qt) & 1ull) + (nt - 1) * (qt & 1ull);", "if (nt) T += (qt & 1ull) + (nt - 1) * (qt & 1ull);", 1, False),
    ("mode 3: (cnt - odd) : odd swapped", "((qt & 1ull) ? (cnt - odd) : odd)", "((qt & 1ull) ? odd : (cnt - odd))", 1, False),
    ("up_first without the distance (jt - i) & 1", "up_first = (p + (uint64_t)((jt - i) & 1) + qt) & 1ull;", "up_first = (p + qt) & 1ull;", 1, False),
    ("odd_before(om, po, jt + 1) -> (..., jt)", "odd_before(om, po, jt + 1) : 0;", "odd_before(om, po, jt) : 0;", 1, False),
    ("m > jt -> m >= jt", "if (m > jt) {", "if (m >= jt) {", 1, False),
    ("low_mask off by one", "return b ? (0xffffffffu >> (32 - b)) : 0u;", "return b ? (0xffffffffu >> (31 - b)) : 0u;", 1, False),
    ("first_symbol without the final clamp to n (equivalent)", "return j < B.n ? j : B.n;", "return j;", 1, True),
]
RANGES = (("landing", V.LANDING), ("saturation", V.SATURATION), ("half_ulp", V.HALF_ULP), ("constructed", V.CONSTRUCTED))


def main():
    text = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_twoval.h")).read()
    cases = [V.case(*k) for k in V.case_list()]
    rows, wrong = [], []
    for name, old, new, times, equivalent in MUTATIONS:
        assert text.count(old) == times, (name, text.count(old))
        with tempfile.TemporaryDirectory(prefix="twoval_mut_") as d:
            with open(os.path.join(d, "amwg_twoval.h"), "w") as f:
                f.write(text.replace(old, new))
            run = build_host(d, header_dir=d)
            total, failing, by_flag, by_range = 0, 0, {f: 0 for f in V.LANE_FLAGS}, {r: 0 for r, _ in RANGES}
            for c in cases:
                bad = ~V.same_bits(run(c["n"], c["tab"], c["acc0"], c["l1"], c["l0"]), c["want"])
                total += int(bad.sum())
                failing += bool(bad.any())
                for r, sl in RANGES:
                    by_range[r] += int(bad[sl].sum())
                for f in V.LANE_FLAGS:
                    by_flag[f] += int((bad & c["flags"][f]).sum())
        top = sorted((f for f in V.LANE_FLAGS if by_flag[f]), key=lambda f: -by_flag[f])[:3]
        rows.append("| %s | %d | %d of %d | %s | %s |" % (name, total, failing, len(cases), ", ".join("%s %d" % (r, v) for r, v in by_range.items() if v) or "--",
                                                       ", ".join("%s %d" % (f, by_flag[f]) for f in top) or "--"))
        if (total == 0) != equivalent:
            wrong.append(name)
    print("| mutation | lanes that differ | cases that fail | of them, in the lane ranges | of them, lanes whose census has (a lane may have several) |\n|---|---|---|---|---|")
    print("\n".join(rows))
    print("survived without being equivalent, or caught although listed as equivalent:", wrong or "none")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
