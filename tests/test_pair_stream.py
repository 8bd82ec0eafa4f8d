"""The pair draw of the one-lane stream (csrc/amwg_philox.h stream_next_pair = CoopStream<1>::next_pair of csrc/amwg_kernel.h: the two uniforms of an
rnorm trial with the Philox refill at one call site), compiled for the host: tests/host/pair_stream.cpp runs it on a restatement of the one-lane stream against
ChainStream::next() from each of the three positions, interleaved with single draws in every pattern of length 1 .. 6, over 10^4 uniforms each -- the same
values, the same consumed counts, the same number of refills."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_draws_are_two_single_draws_from_every_position_in_every_pattern(tmp_path):
    exe = str(tmp_path / "pair_stream")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "bayes.js_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "pair_stream.cpp"), "-o", exe])
    p = subprocess.run([exe, "10000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "patterns=%d " % (3 * 126) in p.stdout and "failures=0" in p.stdout, p.stdout[-2000:]
