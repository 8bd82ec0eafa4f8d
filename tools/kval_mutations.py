#!/usr/bin/env python3
"""tools/kval_mutations.py -- do the cases of tests/kval_cases.py discriminate?  Applies one small mutation at a time to a temporary copy of csrc/amwg_kval.h,
builds tests/host/kval_eval_host.cpp against the copy FOR THE HOST (nothing is written into the tree, nothing runs on a GPU) and counts the lanes whose sum
differs from the plain sequential sum, by census class.  Prints the table of tests/README.kval.md.  Exit status 1 if a mutation that is not listed as
equivalent survives.      python tools/kval_mutations.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kval_cases as V      # noqa: E402
from test_kval_host import build_host      # noqa: E402

MUTATIONS = [
    ("tie rounds up: r > h -> r >= h", "(r > h ? 1u : 0u)", "(r >= h ? 1u : 0u)", False),
    ("`^ QB` dropped from up", "(prev_cov & (X ^ prev_val ^ QB)) | (~prev_cov & (X ^ PIN ^ QB))", "(prev_cov & (X ^ prev_val)) | (~prev_cov & (X ^ PIN))", False),
    ("prev_cov without << 1", "prev_cov = m << 1;", "prev_cov = m;", False),
    ("limit larger by one", "const uint64_t limit = (1ull << 53) - A;", "const uint64_t limit = (1ull << 53) - A + 1;", False),
    # equivalent in its results: at e == emax the largest addend has s = 0, so d = its whole significand (exact, no remainder, no tie) >= 2^52 >= limit -- the
    # bisection and the block walk both stop in front of its first occurrence and the real addition does the rest; the smaller addends have s >= 1 as before.  What
    # the header's `+ 1` buys is that `1ull << (s - 1)` is never a shift by -1 (undefined in C++; the hardware masks the count and r == h, r > h stay false)
    ("e >= emax + 1 -> e >= emax (equivalent: see the comment)", "if (!(e >= emax + 1 && e < 0x7ff))", "if (!(e >= emax && e < 0x7ff))", True),
    ("s >= 54 -> s >= 53", "if (s >= 54) d[k] = 0;", "if (s >= 53) d[k] = 0;", False),
    # equivalent: a product with hi in [2^21, 2^22) is (hi << 32) + ... >= 2^53 > limit (<= 2^52) without overflow, and growth() saturates it on `t >= limit`
    ("hi >> 21 -> hi >> 22 (equivalent: see the comment)", "if (hi >> 21) return kSat;", "if (hi >> 22) return kSat;", True),
    ("saturation of n * d removed (hi << 32 wraps)", "if (hi >> 21) return kSat;", "", False),
    ("block walk: break test off by one", "if (A_new >= (1ull << 53)) break;", "if (A_new > (1ull << 53)) break;", False),
    ("fill-forward: last doubling dropped", "v |= (v << 16) & ~m; m |= m << 16;", "", False),
    ("count_before ignores the partial block", "& low_mask(m & 31));", "& 0u);", False),
]


def main():
    text = open(os.path.join(ROOT, "bayes.js_amd", "csrc", "amwg_kval.h")).read()
    cases = [V.case(*k) for k in V.case_list()]
    rows, survived = [], []
    for name, old, new, equivalent in MUTATIONS:
        assert text.count(old) == 1, (name, text.count(old))
        with tempfile.TemporaryDirectory(prefix="kval_mut_") as d:
            with open(os.path.join(d, "amwg_kval.h"), "w") as f:
                f.write(text.replace(old, new))
            run = build_host(d, header_dir=d)
            total, by_flag, failing, landing = 0, {f: 0 for f in V.LANE_FLAGS}, 0, 0
            for c in cases:
                bad = ~V.same_bits(run(c["K"], c["idx"], c["tab"], c["acc0"], c["c"]), c["want"])
                total += int(bad.sum())
                failing += bool(bad.any())
                landing += int(bad[V.LANDING].sum())
                for f in V.LANE_FLAGS:
                    by_flag[f] += int((bad & c["flags"][f]).sum())
        top = sorted((f for f in V.LANE_FLAGS if by_flag[f]), key=lambda f: -by_flag[f])[:3]
        rows.append("| %s | %d | %d of %d | %d | %s |" % (name, total, failing, len(cases), landing, ", ".join("%s %d" % (f, by_flag[f]) for f in top) or "--"))
        if total == 0 and not equivalent:
            survived.append(name)
    print("| mutation | lanes that differ | cases that fail | of them, landing lanes | of them, lanes whose census has (a lane may have several) |\n|---|---|---|---|---|")
    print("\n".join(rows))
    print("survived:", survived or "none")
    return 1 if survived else 0


if __name__ == "__main__":
    sys.exit(main())
