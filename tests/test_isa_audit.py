"""The gfx950 code objects of the benched step-kernel instantiations carry no spilled VGPR and no scratch traffic inside their loops
(tools/isa_audit.py: hipcc cross-compiles here, no GPU needed).  Round 2 compiled every instantiation for 1024-thread workgroups and
carried 31 scratch instructions through the slot loop of the cfg4 kernel."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_benched_kernels_have_no_vgpr_spills_or_scratch_in_their_loops():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_audit.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert "isa audit ok" in p.stdout
    # (the inline scalar loads of the certified pass: every one waited for before use, in the certified Normal kernels and a closure's certified tail)
    m = re.search(r"inline s_load_dwordx16 waited for .*: (.*)", p.stdout)
    assert m, p.stdout[-2000:]
    counts = dict((k, int(v)) for k, v in re.findall(r"(\S+) (\d+)(?:,|$)", m.group(1)))
    want = ["NormalModel,1,256,cert", "NormalModel,1,512,cert"] + (["amwg_user_step_cert(bench_normal,1,256)"] if shutil.which("node") else [])
    assert all(counts.get(k, 0) > 0 for k in want), counts


# ---- the inline scalar-load rule (tools/isa_audit.py inline_smem_waits) on synthetic assembly: it must pass clean code and catch each way of using a
# load's registers before its wait
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_audit  # noqa: E402

_CLEAN = """
	;;#ASMSTART
	s_load_dwordx16 s[20:35], s[4:5], 0x40
	;;#ASMEND
	v_mov_b32_e32 v0, s10
	v_fma_f64 v[2:3], v[4:5], s[36:37], v[2:3]
	;;#ASMSTART
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	v_mov_b32_e32 v1, s21
	s_cbranch_scc1 .LBB0_2
.LBB0_2:
	s_endpgm
"""


def test_inline_load_rule_passes_a_load_waited_for_before_use():
    assert isa_audit.inline_smem_waits(_CLEAN.splitlines()) == (1, [])


@pytest.mark.parametrize("early", ["\tv_mov_b32_e32 v1, s21\n",                      # reads a destination register
                                   "\tv_fma_f64 v[2:3], s[34:35], v[4:5], v[2:3]\n",   # reads the last pair of the range
                                   "\ts_mov_b32 s20, 0\n",                             # writes one
                                   "\ts_waitcnt lgkmcnt(1)\n\tv_mov_b32_e32 v1, s22\n",  # a partial wait does not count
                                   ".LBB0_1:\n",                                       # a label: another path may reach the use
                                   "\ts_branch .LBB0_2\n"])
def test_inline_load_rule_catches_a_register_touched_before_the_wait(early):
    asm = _CLEAN.replace("\tv_mov_b32_e32 v0, s10\n", "\tv_mov_b32_e32 v0, s10\n" + early)
    n, bad = isa_audit.inline_smem_waits(asm.splitlines())
    assert n == 1 and len(bad) == 1, bad


def test_inline_load_rule_ignores_compiler_loads_and_counts_none_without_inline_ones():
    asm = _CLEAN.replace(";;#ASMSTART\n\ts_load_dwordx16", "s_load_dwordx16", 1).replace("0x40\n\t;;#ASMEND", "0x40", 1)
    assert "ASMSTART\n\ts_load" not in asm
    assert isa_audit.inline_smem_waits(asm.splitlines()) == (0, [])
