"""Certified Poisson / logistic tails for a translated closure on MANY datasets (translate.js translate_datasets with tail_consts_array; csrc/amwg_gtail.h:
kTailPerDataset), the part that needs no GPU: the one source carries the tail and the marker, the data-dependent constants of its bound are slots of one
more array per dataset -- EACH dataset's own, which is what a device run cannot see: a bound formed from dataset 0's values for everyone still decides nearly every test
the same way --, a dataset that cannot take the plan sends all of them back to the expression, the source compiles for gfx950 with the certified dataset twin, evaluates
to the closure's value under Node on every dataset, and what the library refuses it refuses before a device is opened.  Fixtures: tests/js/dataset_tail_models.js.

dst_pois_small has 37 observations.  An ORDINARY translation emits these plans from 64 observations on (translate.js forLoop), so that fixture's own translations carry
no literals to compare with; its slots are checked against the sums and maxima formed here from the arrays, as every Poisson fixture's are.  In the per-dataset form the
plan is emitted at any size: segments are short."""
import copy
import math
import re
import struct

import numpy as np
import pytest

import amwg_ctypes
import user_dataset_tails_lib as tl
import user_datasets_lib as udl

pytestmark = [pytest.mark.node, pytest.mark.skipif(udl.NODE is None, reason="node is not installed")]
N_OBS = {"dst_logit": 517, "dst_logit_weights": 517, "dst_pois_linear": 65, "dst_pois_small": 37}


def bits(v):
    return struct.pack(">d", float(v)).hex()


def literal(text):
    """a number as translate.js hexFloat writes it: `150.0`, or a C99 hexadecimal literal"""
    text = text.strip()
    return float.fromhex(text) if "0x" in text else float(text)


def is_logit(tag):
    return tag.startswith("dst_logit")


@pytest.mark.parametrize("tag", tl.MARKED)
def test_one_source_with_the_tail_and_the_per_dataset_marker(tag):
    source, meta, sets = tl.load(tag)
    n = N_OBS[tag]
    assert "static constexpr bool kTailPerDataset = true;" in source and "kCertifiedLanes = 16" in source and ("kTailN = %d," % n) in source
    if is_logit(tag):
        assert "kLogitTail = true" in source and "kPoisTail" not in source
        assert meta["logit_tail_n"] == n and meta["pois_tail_n"] == 0
        want_len = 1
    else:
        assert "kPoisTail = true" in source and "kTailLinear = true" in source and "kLogitTail" not in source
        assert meta["pois_tail_n"] == n and meta["logit_tail_n"] == 0
        want_len = 2 + 3
    assert meta["tail_per_dataset"] is True and meta["n_datasets"] == 3
    j = len(meta["array_keys"]) - 1
    assert meta["array_keys"][j] == "#tail:consts" and meta["array_types"][j] == 0 and meta["array_len"][j] == want_len
    assert ("static constexpr int kTailConsts = %d;" % j) in source
    assert all(s[j].size == want_len for s in sets)
    # never staged: the LDS plan is that of the same closure without the tail
    off = tl.load(tag + ".notail")[1]
    assert meta["lds_bytes"] == off["lds_bytes"] and meta["lds_bytes_one_lane"] == off["lds_bytes_one_lane"]
    assert off["array_keys"] == meta["array_keys"][:-1]
    # no literal of the bound in the text, and the accessors take the data reference
    assert "gtail_sum_y()" not in source and "gtail_sum_lf()" not in source and "gtail_hlin(const StateView &S)" not in source
    if is_logit(tag):
        assert "gtail_sum_y(const DataRef &d)" in source
    else:
        assert "gtail_sum_y(const DataRef &d)" in source and "gtail_sum_lf(const DataRef &d)" in source and "gtail_hlin(const StateView &S, const DataRef &d)" in source


def neumaier(values):
    s = c = 0.0
    for v in values:
        t = s + v
        c += (s - t) + v if abs(s) >= abs(v) else (v - t) + s
        s = t
    return s + c


def formed_here(tag, meta, arrays):
    """the slots from the arrays, by the rules the headers state: sum y exact, sum lfactorial compensated, column maxima; sum |y| rounded up unless an integer"""
    key = {k: j for j, k in enumerate(meta["array_keys"])}
    if is_logit(tag):
        y = arrays[key[".w" if tag == "dst_logit_weights" else ".y"]]
        s = 0.0
        for v in y:
            s += abs(float(v))
        if not float(s).is_integer():
            s *= 1 + y.size * 2.0 ** -52
        return [s]
    y, X = arrays[key[".y"]], arrays[key[".X"]].reshape(-1, 3)
    lf = arrays[[j for k, j in key.items() if k.startswith("#aux:lfactorial")][0]]
    assert all(abs(float(a) - math.lgamma(float(v) + 1.0)) <= 1e-12 * (1.0 + abs(float(a))) for a, v in zip(lf, y))
    return [float(sum(int(v) for v in y)), neumaier([float(v) for v in lf])] + [float(np.abs(X[:, k]).max()) for k in range(3)]


@pytest.mark.parametrize("tag", tl.MARKED)
def test_the_constants_are_each_datasets_own(tag):
    source, meta, sets = tl.load(tag)
    j = len(meta["array_keys"]) - 1
    slot_of_state = {int(si): int(slot) for slot, si in re.findall(r"tail_const\(c_, (\d+)\) \* __builtin_fabs\(S\((\d+)\)\)", source)}
    if not is_logit(tag):
        assert slot_of_state == {0: 2, 1: 3, 2: 4}      # every column's term, whatever its maximum
    seen = []
    for d in range(3):
        got = [float(v) for v in sets[d][j]]
        print(tag, d, got)
        assert [bits(v) for v in got] == [bits(v) for v in formed_here(tag, meta, sets[d])], (tag, d)
        own = tl.load_own(tag, d)[0]
        if N_OBS[tag] >= 64:      # (the ordinary translation has the plan, with literals)
            if is_logit(tag):
                m = re.search(r"gtail_sum_y\(\) \{ return ([^;]+); \}", own)
                assert m and bits(literal(m.group(1))) == bits(got[0]), (tag, d)
            else:
                my, mf = re.search(r"gtail_sum_y\(\) \{ return ([^;]+); \}", own), re.search(r"gtail_sum_lf\(\) \{ return ([^;]+); \}", own)
                assert my and mf and bits(literal(my.group(1))) == bits(got[0]) and bits(literal(mf.group(1))) == bits(got[1]), (tag, d)
                hl = re.search(r"gtail_hlin\(const StateView &S\) \{ return ([^;]+); \}", own).group(1)
                factors = {int(si): literal(lit) for lit, si in re.findall(r"([-+.\w]+) \* __builtin_fabs\(S\((\d+)\)\)", hl)}
                for si, slot in slot_of_state.items():
                    assert bits(got[slot]) == bits(factors.get(si, 0.0)), (tag, d, si)      # (a column whose own translation pruned the term: slot 0)
                if tag == "dst_pois_linear" and d == 2:
                    assert 1 not in factors and got[3] == 0.0 and got[4] > 7.0
        else:
            assert "kPoisTail" not in own and "kLogitTail" not in own
        seen.append(tuple(bits(v) for v in got))
    for a in range(3):
        for b in range(a + 1, 3):
            assert all(x != y for x, y in zip(seen[a], seen[b])), (tag, a, b, seen)      # every slot differs between the datasets


def test_the_constants_may_be_the_17th_array():
    """dst_logit_many: 16 data arrays, so `#tail:consts` is array 16 -- past the pointers that travel in the kernel arguments, read through the device table"""
    source, meta, sets = tl.load("dst_logit_many")
    assert meta["array_keys"][16] == "#tail:consts" and len(meta["array_keys"]) == 17 and meta["logit_tail_n"] == 65
    assert "static constexpr int kTailConsts = 16;" in source and "tail_const(user_arr<16>(d), 0)" in source
    assert [float(s[16][0]) for s in sets] == [float(s[meta["array_keys"].index(".y")].sum()) for s in sets]
    h = tl.host_eval("dst_logit_many")
    for k in range(3):
        for state, want in zip(h.meta["states"][k], h.meta["log_post"][k]):
            assert bits(h.eval(k, state, lanes=1)[0]) == want, (k, state)


def test_storage_type_is_the_union():
    _, meta, sets = tl.load("dst_pois_linear")
    j = meta["array_keys"].index(".y")
    assert meta["array_types"][j] == 2 and sets[1][j].max() >= 200 and sets[0][j].max() <= 5      # i32 for all: dataset 1's counts
    assert [tl.load_own("dst_pois_linear", d)[1]["array_types"][0] for d in range(3)] == [1, 2, 1]


def test_a_dataset_that_cannot_take_the_plan_sends_all_back_to_the_expression():
    source, meta, _ = tl.load("dst_pois_fallback")
    off_source, off_meta, _ = tl.load("dst_pois_fallback.notail")
    assert meta["pois_tail_n"] == 0 and meta["tail_per_dataset"] is False and "kPoisTail" not in source and "kTailPerDataset" not in source
    assert "#tail:consts" not in meta["array_keys"]
    assert source == off_source and meta["array_keys"] == off_meta["array_keys"]


@pytest.mark.parametrize("tag", ["dst_logit", "dst_pois_linear"])
def test_the_callers_switch_gives_the_source_without_these_tails(tag):
    """{no_logit_tail: true} / {no_pois_tail: true}: tailless, and the text of the same input under the options translate_datasets forced on every pass before it
    knew these tails (no_pois_tail, no_logit_tail, no_row_plan, no_const_element_fold)"""
    source, meta, _ = tl.load(tag + ".notail")
    assert meta["logit_tail_n"] == 0 and meta["pois_tail_n"] == 0 and meta["tail_per_dataset"] is False
    assert "kLogitTail" not in source and "kPoisTail" not in source and "kTailPerDataset" not in source and "tail_const" not in source
    assert source == tl.forced_source(tag)
    assert source != tl.load(tag)[0]


@pytest.mark.parametrize("tag", tl.MARKED)
def test_marked_source_compiles_for_gfx950_with_the_certified_twin(tag, tmp_path, monkeypatch):
    import ctypes as C
    L = amwg_ctypes.lib()
    dump = tmp_path / "code.hsaco"
    monkeypatch.setenv("AMWG_DUMP_CODE_OBJECT", str(dump))
    n = C.c_size_t(0)
    rc = L.amwg_compile_user_datasets(tl.load(tag)[0].encode(), 16, 64, b"gfx950", C.byref(n))
    assert rc == 0, L.amwg_last_error().decode()[-3000:]
    code = dump.read_bytes()
    assert len(code) == n.value > 0 and b"amwg_user_step_cert_ds" in code and b"amwg_user_step_ds" in code


@pytest.mark.parametrize("tag", tl.MARKED)
def test_host_build_equals_the_closure_under_node_on_every_dataset(tag):
    h = tl.host_eval(tag)
    seen = set()
    for k in range(3):
        for state, want in zip(h.meta["states"][k], h.meta["log_post"][k]):
            got, _ = h.eval(k, state, lanes=1)
            print(tag, k, bits(got), want)
            assert bits(got) == want, (tag, k, state)
            seen.add(want)
    assert len(seen) == 15


def refused(spec_list, why, chains=12):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(spec_list, chains=chains, seed=1, lanes_per_chain=16, block_threads=64)
    msg = str(ei.value)
    assert "amwg error -1" in msg, msg      # AMWG_EINVAL: before a device was needed
    assert re.search(why, msg), msg


@pytest.mark.parametrize("tag,why", [("dst_pois_linear", r"certified Poisson tail \(kPoisTail\)"), ("dst_logit", r"certified logistic tail \(kLogitTail\)")])
def test_refusals_before_a_device_is_opened(tag, why):
    refused(copy.deepcopy(tl.specs(tag)), r"amwg_create_user_datasets: chains \(13, the total\) must be a multiple of n_datasets \(3\)", chains=13)
    s = copy.deepcopy(tl.specs(tag))
    for q in s:
        assert q["user"]["source"].count("  static constexpr bool kTailPerDataset = true;\n") == 1
        q["user"]["source"] = q["user"]["source"].replace("  static constexpr bool kTailPerDataset = true;\n", "")
    refused(s, why)
