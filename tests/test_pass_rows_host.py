"""The row plan of the wavefront's certified pass (csrc/amwg_pass.h pass_rows, pass_part_slot, pass_part_row -- the helpers norm_sq_pass_wave walks by),
compiled for the host: tests/host/pass_rows.cpp follows the kernel's order of blocks, remainder parts and the partly filled row for every n from 1 to
4 * 1024 + 65 and blocks of 8 and 16 rows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_observation_is_covered_once_and_one_block_at_most_is_short(tmp_path):
    exe = str(tmp_path / "pass_rows")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "pass_rows.cpp"), "-o", exe])
    p = subprocess.run([exe, str(4 * 1024 + 65)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "checked=%d failures=0" % (2 * (4 * 1024 + 65)) in p.stdout, p.stdout[-2000:]
