#!/usr/bin/env python3
"""tools/user_isa.py NAME [LANES | LANESxBLOCK ...] -- what the gfx950 compiler makes of a TRANSLATED closure's step kernels (no GPU needed).
Translates tests/js/user_models.js:NAME, compiles the program csrc/amwg_rtc.hip would hand to hiprtc (isa_audit.user_asm) with hipcc -S and lists
the innermost loops of amwg_user_step by VALU count (the likelihood loop's unrolled body is the largest) -- and of amwg_user_step_cert where the closure has
certified decisions at that lane count (csrc/amwg_gtail.h: the wavefront's pass is its largest loop)."""
import os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "bayes.js_amd")]
import isa_audit
import user_host

name = sys.argv[1]
lanes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[2:]] or [(64,)]
src, arrays, meta = user_host.translated(name)
for geo in lanes:
    G, block = geo[0], geo[1] if len(geo) > 1 else min(256, meta["max_threads"])
    out = isa_audit.user_asm(src, G, block)
    txt = open(out).read()
    meta_k = isa_audit.kernel_metadata(txt)
    for kernel in ("amwg_user_step", "amwg_user_step_cert"):
        if kernel not in meta_k or meta_k[kernel]["vgpr"] <= 8:      # (a _cert kernel without a body: the closure has no certified decisions at this lane count)
            continue
        print(name, "G=%d block=%d" % (G, block), kernel, meta_k.get(kernel), out)
        # innermost loops
        ins, labels = [], {}
        body = False
        for ln in txt.splitlines():
            if ln.startswith(kernel + ":"):
                body = True
                continue
            if not body:
                continue
            if ln.startswith(".Lfunc_end"):
                break
            s = ln.split(";")[0].strip()
            if not s:
                continue
            m = re.match(r"^(\.L\w+):", s)
            if m:
                labels[m.group(1)] = len(ins)
                continue
            if s.startswith("."):
                continue
            ins.append(s)
        loops = []
        for i, s in enumerate(ins):
            m = re.match(r"^s_c?branch\w*\s+(\.L\w+)", s)
            if m and m.group(1) in labels and labels[m.group(1)] <= i:
                loops.append((labels[m.group(1)], i))
        inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
        if os.environ.get("ALL_LOOPS"):
            inner = loops
        rows = []
        for a, b in inner:
            seg = ins[a:b + 1]
            c = lambda pred: sum(1 for s in seg if pred(s.split()[0]))
            rows.append((c(lambda o: o.startswith("v_")), c(lambda o: "f64" in o), c(lambda o: o.startswith("s_") and not o.startswith("s_waitcnt")),
                         c(lambda o: o.startswith("ds_")), c(lambda o: o.startswith("global_") or o.startswith("flat_")), c(lambda o: o.startswith("s_cbranch") or o.startswith("s_branch")),
                         c(lambda o: o in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64")), c(lambda o: o == "v_rcp_f64_e32" or o == "v_rcp_f64_e64"), a, b))
        rows.sort(reverse=True)
        print("  innermost loops by VALU:  valu  f64  salu  ds  global  branches  div_pieces  rcp  [first..last instruction]")
        for r in rows[:6]:
            print("   ", r)
