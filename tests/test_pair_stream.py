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
    # the same comparison under keys with every word in use, from first uniforms on either side of the carry of the block number into its high word (uniform
    # 2^33) -- runs that begin before it and cross it, begin on it, begin after it.  Both sides are host builds of the product's code: the value ChainStream gives
    # at the carry is pinned to the numpy twin as well.
    import synth
    for seed, chain in ((0x9E3779B97F4A7C15, 2 ** 32 - 3 + 5), (2 ** 64 - 1, 2 ** 63 + 5), (2 ** 32, 2 ** 32)):
        for base in (2 ** 33 - 40, 2 ** 33 - 2, 2 ** 33, 2 ** 33 + 4):
            p = subprocess.run([exe, "96", str(base), str(seed), str(chain), str(2 ** 33 + 1)], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0 and "patterns=%d " % (3 * 126) in p.stdout and "failures=0" in p.stdout, (hex(seed), hex(chain), base, p.stdout[-2000:])
            assert "uniform=%016x\n" % int(synth.uniforms(seed, chain, 2, 2 ** 33)[1:].view("<u8")[0]) in p.stdout, (hex(seed), hex(chain), p.stdout[-300:])
