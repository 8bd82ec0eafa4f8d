"""Many datasets in one sampler for a TRANSLATED closure (translate.js translate_datasets, amwg_create_user_datasets), the part that needs no GPU: one source for
all datasets under the union of what their values decide, that source evaluated on every dataset's arrays equals the closure under Node bit for bit, what cannot be
one source is refused with a message that says why, the dataset twins compile for gfx950 (and only where asked for), and every call the library refuses is refused
BEFORE a device is opened."""
import copy
import os
import re
import struct
import subprocess

import pytest

import amwg_ctypes
import user_datasets_lib as udl

ROOT = udl.ROOT
pytestmark = [pytest.mark.node, pytest.mark.skipif(udl.NODE is None, reason="node is not installed")]
MODELS = ["ds_scaled_normal", "ds_readme_normal", "ds_mixed", "ds_many_arrays"]


def bits(v):
    return struct.pack(">d", v).hex()


@pytest.mark.parametrize("tag", MODELS)
def test_one_source_and_arrays_of_equal_shape(tag):
    source, meta, sets = udl.load(tag)
    assert meta["n_datasets"] == udl.D == len(sets)
    for arrays in sets:
        assert [a.size for a in arrays] == meta["array_len"] and len(arrays) == len(meta["array_types"])
    # nothing in the one source that is formed from one dataset's values
    assert "kRowN" not in source and "kPoisTail = true" not in source and "kLogitTail = true" not in source
    assert meta["rows_n_obs"] == 0 and meta["pois_tail_n"] == 0 and meta["logit_tail_n"] == 0


def test_readme_normal_keeps_its_certified_tail():
    source, meta, _ = udl.load("ds_readme_normal")
    assert "kCertifiedTail = true" in source and meta["cert_tail_n"] == 37


def test_union_of_types_and_ranges():
    """ds_mixed: y is u8 in dataset 0, i32 in dataset 1 (one 300), f64 in dataset 2 (one 2.5): f64 for all.  g is {0, 1} in dataset 0, {0, 1, 2} in the others: u8,
    range [0, 2].  Each dataset's OWN translation shows that the datasets really differ."""
    _, meta, sets = udl.load("ds_mixed")
    key = {k: j for j, k in enumerate(meta["array_keys"])}
    own = [udl.load_own("ds_mixed", k)[1] for k in range(3)]
    assert [o["array_types"][o["array_keys"].index(".y")] for o in own] == [amwg_ctypes_type("u8"), amwg_ctypes_type("i32"), amwg_ctypes_type("f64")]
    assert meta["array_types"][key[".y"]] == amwg_ctypes_type("f64") and meta["array_ranges"][key[".y"]] is None
    assert meta["array_types"][key[".g"]] == amwg_ctypes_type("u8") and meta["array_ranges"][key[".g"]] == [0, 2]
    assert sets[0][key[".g"]].max() == 1 and sets[1][key[".g"]].max() == 2
    assert meta["array_types"][key[".x"]] == amwg_ctypes_type("f64")
    assert not any(meta["array_is01"])


def amwg_ctypes_type(name):
    return {"f64": 0, "u8": 1, "i32": 2}[name]      # AMWG_F64 / AMWG_U8 / AMWG_I32 (include/amwg.h)


def test_varying_scalar_is_an_array_and_an_equal_one_is_folded():
    source, meta, sets = udl.load("ds_mixed")
    assert meta["varying_scalars"] == [".offset"]
    j = meta["array_keys"].index("#scalar:.offset")
    assert meta["array_types"][j] == 0 and meta["array_len"][j] == 1
    assert [float(s[j][0]) for s in sets] == [-0.25, -0.125, 0.0]
    assert "A%d[0]" % j in source
    assert not any(k.startswith("#scalar:.scale") for k in meta["array_keys"]) and "* 0x1.0000000000000p-1)" in source      # data.scale = 0.5 in every dataset: a literal


@pytest.mark.parametrize("tag", MODELS)
def test_host_build_equals_the_closure_under_node_on_every_dataset(tag):
    """bit for bit, 5 states per dataset, one lane per chain (the reference's order), the derived quantities too"""
    h = udl.HostEval(tag)
    meta = h.meta
    seen = set()
    for k in range(udl.D):
        for state, want, want_dv in zip(meta["states"][k], meta["log_post"][k], meta["derived_values"][k]):
            got, dv = h.eval(k, state, lanes=1)
            print(tag, k, bits(got), want)
            assert bits(got) == want or (got != got and struct.unpack(">d", bytes.fromhex(want))[0] != struct.unpack(">d", bytes.fromhex(want))[0]), (tag, k, state)
            assert [bits(v) for v in dv] == want_dv, (tag, k, state)
            seen.add(want)
    assert len(seen) > udl.D      # (the datasets and the states really differ)


def test_translate_datasets_refuses_what_cannot_be_one_source():
    r = udl.refusals()
    assert r["bad_shapes"] and re.search(r"equal shape: data has dimensions \[5\] in dataset 1 and \[4\] in dataset 0", r["bad_shapes"]), r["bad_shapes"]
    assert r["bad_loop_bound"] and re.search(r"the bound of the loop over i is data\.n, whose value differs between the datasets", r["bad_loop_bound"]), r["bad_loop_bound"]
    assert "dataset 0" in r["bad_loop_bound"]
    m = r["bad_levels"]
    assert m and re.search(r"the source of dataset 1 differs from dataset 0's at line \d+:", m) and "dataset 0: " in m and "dataset 1: " in m and "strings with different levels" in m, m


@pytest.mark.parametrize("tag", ["ds_scaled_normal", "ds_readme_normal"])
@pytest.mark.parametrize("lanes,block", [(1, 64), (16, 64)])
def test_dataset_twins_compile_for_gfx950_and_only_when_asked(tag, lanes, block, tmp_path, monkeypatch):
    import ctypes as C
    source = udl.load(tag)[0].encode()
    L = amwg_ctypes.lib()
    dump = tmp_path / "code.hsaco"
    monkeypatch.setenv("AMWG_DUMP_CODE_OBJECT", str(dump))
    n = C.c_size_t(0)
    rc = L.amwg_compile_user_datasets(source, lanes, block, b"gfx950", C.byref(n))
    assert rc == 0, L.amwg_last_error().decode()[-3000:]
    code = dump.read_bytes()
    assert len(code) == n.value > 0 and b"amwg_user_step_ds" in code and b"amwg_user_step_cert_ds" in code and b"amwg_user_step\0" in code
    if (lanes, block) == (1, 64):      # (one geometry is enough for the converse)
        rc = L.amwg_compile_user(source, lanes, block, b"gfx950", C.byref(n))
        assert rc == 0, L.amwg_last_error().decode()[-3000:]
        plain = dump.read_bytes()
        assert len(plain) == n.value and b"amwg_user_step\0" in plain and b"_ds" not in plain.replace(b"_dsp", b"")


# ---- amwg_create_user_datasets: refused before a device is opened
def refused(spec_list, why, chains=12, **opts):
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(spec_list, chains=chains, seed=1, **opts)
    msg = str(ei.value)
    assert "amwg error -1" in msg, msg      # AMWG_EINVAL: not AMWG_EHIP, i.e. before a device was needed
    assert re.search(why, msg), msg


def fresh(tag="ds_mixed"):
    return copy.deepcopy(udl.specs(tag))


def test_null_argument_and_no_datasets_are_refused():
    import ctypes as C
    L = amwg_ctypes.lib()
    um, pa, oa, op, h = (amwg_ctypes.UserModel * 2)(), (amwg_ctypes.ParamDesc * 2)(), (amwg_ctypes.CompOpt * 2)(), amwg_ctypes.Options(), C.c_void_p()
    init = (C.c_double * 2)(0.5, 0.5)
    op.chains = 12
    for n in (0, -3):
        assert L.amwg_create_user_datasets(um, n, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1
        assert b"n_datasets must be >= 1" in L.amwg_last_error()
    assert L.amwg_create_user_datasets(None, 2, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1 and b"null argument" in L.amwg_last_error()
    assert L.amwg_create_user_datasets(um, 2, pa, 2, init, oa, C.byref(op), C.byref(h)) == -1      # (no source)
    assert b"null argument (dataset 0: source)" in L.amwg_last_error()
    assert L.amwg_compile_user_datasets(None, 1, 64, b"gfx950", None) == -1 and b"null argument" in L.amwg_last_error()


def test_chains_must_be_a_multiple_of_the_datasets():
    refused(fresh(), r"amwg_create_user_datasets: chains \(13, the total\) must be a multiple of n_datasets \(3\)", chains=13)


def test_a_different_source_is_refused():
    s = fresh()
    s[2]["user"]["source"] += "\n// another text\n"
    refused(s, r"dataset 2: source differs from dataset 0's")


def test_a_different_layout_is_refused():
    s = fresh()
    s[1]["user"]["arrays"] = s[1]["user"]["arrays"][:-1]
    s[1]["user"]["array_types"] = s[1]["user"]["array_types"][:-1]
    refused(s, r"dataset 1: n_arrays = 4, dataset 0 has 5")
    s = fresh()
    s[1]["user"]["arrays"][0] = s[1]["user"]["arrays"][0][:-1]
    refused(s, r"dataset 1: array_len\[0\] = 69, dataset 0 has 70 .*equal shape")
    s = fresh()
    s[2]["user"]["array_types"] = [t if j != 1 else 2 for j, t in enumerate(s[2]["user"]["array_types"])]      # (a list of its own: the specs share the meta's)
    refused(s, r"dataset 2: array_type\[1\] = 2, dataset 0 has 1")
    for field, other in (("n_derived", 0), ("lds_bytes", 16), ("lds_bytes_one_lane", 16), ("parallel", 0), ("max_threads", 64), ("rows_n_obs", 64), ("rows_groups", 2), ("rows_sweep", 1)):
        s = fresh()
        s[1]["user"][field] = other
        refused(s, r"dataset 1: %s = %d, dataset 0 has \d+" % (field, other))


def test_sources_formed_from_one_datasets_values_are_refused():
    for marker, why in (("static constexpr int kRowN = 64;", r"the source has a row plan \(kRowN\)"),
                        ("static constexpr bool kPoisTail = true; static constexpr int kTailN = 70;", r"certified Poisson tail \(kPoisTail\)"),
                        ("static constexpr bool kLogitTail = true; static constexpr int kTailN = 70;", r"certified logistic tail \(kLogitTail\)")):
        s = fresh()
        for q in s:
            q["user"]["source"] += "\n// " + marker + "\n"
        refused(s, why)


def test_autotune_and_sufficient_statistics_are_refused():
    refused(fresh(), r"amwg_create_user_datasets: AMWG_LANES_AUTOTUNE is not supported", lanes_per_chain=-2)
    refused(fresh(), r"sufficient_statistics: only the built-in Normal family", sufficient_statistics=1)


def test_a_list_mixing_a_closure_and_a_family_is_an_error():
    import model_spec
    s = fresh()
    s[1] = model_spec.build_spec("normal", model_spec.make_data("normal", 40, 7))
    with pytest.raises(amwg_ctypes.AmwgError) as ei:
        amwg_ctypes.Sampler(s, chains=12, seed=1)
    assert "mix" in str(ei.value)


JS_CASE = r"""
const mcmc = require('./bayes.js_amd/mcmc.js');
const ld = require('./bayes.js_amd/ld.js');
global.ld = ld;
const dm = require('./tests/js/dataset_models.js');
function thrown(f) { try { f(); } catch (e) { return String(e && e.message ? e.message : e); } return null; }
const bad = dm.build('bad_shapes');
let m = thrown(() => new mcmc.AmwgSampler(bad.params, bad.log_post, null, { datasets: bad.datasets, translate: true, chains: 12 }));
if (!m || !/equal shape: data has dimensions \[5\] in dataset 1 and \[4\] in dataset 0/.test(m)) { console.log('FAIL unequal shapes: ' + m); process.exit(1); }
// without the switch the refusal stays, and now names the switch and the condition
const ok = dm.build('ds_scaled_normal');
m = thrown(() => new mcmc.AmwgSampler(ok.params, ok.log_post, null, { datasets: ok.datasets, chains: 12 }));
if (!m || !/options\.datasets/.test(m) || !/built-in/.test(m) || !/translate: true/.test(m) || !/equal shape/.test(m)) { console.log('FAIL without the switch: ' + m); process.exit(1); }
m = thrown(() => new mcmc.AmwgSampler(ok.params, ok.log_post, null, { datasets: ok.datasets, translate: true, chains: 13 }));
if (!m || !/multiple of the 3 datasets/.test(m)) { console.log('FAIL chains: ' + m); process.exit(1); }
console.log('user datasets frontend ok');
"""


def test_js_front_end_hands_on_the_translators_refusal(tmp_path):
    script = tmp_path / "user_datasets_cases.js"
    script.write_text(JS_CASE.replace("./bayes.js_amd/", os.path.join(ROOT, "bayes.js_amd") + "/").replace("./tests/js/", os.path.join(ROOT, "tests", "js") + "/"))
    p = subprocess.run([udl.NODE, str(script)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "user datasets frontend ok" in p.stdout, p.stdout + "\n" + p.stderr
