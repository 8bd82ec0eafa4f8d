"""ctypes binding of libamwg.so (include/amwg.h) for bench.py and the Python tests.

The product's host language is JavaScript (bayes.js_amd/mcmc.js over the N-API shim); this
binding exists because the driver's bench/test harness is Python.  It carries no logic
beyond marshalling: every computation happens in the HIP library, and loading fails loudly
if the library is missing.
"""
import bisect
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMWG_LIB") or os.path.join(HERE, "csrc", "libamwg.so")   # AMWG_LIB: development builds only
MODEL_ID = {"normal": 1, "beta_bern": 2, "hier_normal": 3, "pois_glm": 4}


class ParamDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("len", C.c_int32), ("top", C.c_int32), ("multidim", C.c_int32),
                ("lower", C.c_double), ("upper", C.c_double)]


class CompOpt(C.Structure):
    _fields_ = [("prop_log_scale", C.c_double), ("max_adaptation", C.c_double), ("initial_adaptation", C.c_double),
                ("target_accept_rate", C.c_double), ("batch_size", C.c_double), ("is_adapting", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [("model", C.c_int32), ("n_obs", C.c_int32), ("x", C.POINTER(C.c_double)), ("y", C.POINTER(C.c_double)),
                ("g", C.POINTER(C.c_int32)), ("G", C.c_int32), ("K", C.c_int32), ("hyper", C.c_double * 8)]


DEFAULT_HYPER = {"normal": [0, 100, 0, 100], "beta_bern": [2, 2], "hier_normal": [0, 100, 0, 100, 10], "pois_glm": [0, 10]}


class Options(C.Structure):
    _fields_ = [("chains", C.c_int64), ("seed", C.c_uint64), ("chain_offset", C.c_uint64), ("device", C.c_int32),
                ("lanes_per_chain", C.c_int32), ("block_threads", C.c_int32), ("steps_per_launch", C.c_int32),
                ("exact_division", C.c_int32), ("group_local", C.c_int32), ("full_evaluation", C.c_int32), ("test_bound_shift", C.c_int32), ("sufficient_statistics", C.c_int32)]


class UserModel(C.Structure):
    _fields_ = [("source", C.c_char_p), ("n_arrays", C.c_int32), ("arrays", C.POINTER(C.POINTER(C.c_double))),
                ("array_len", C.POINTER(C.c_int64)), ("array_type", C.POINTER(C.c_int32)), ("n_derived", C.c_int32), ("lds_bytes", C.c_int32), ("lds_bytes_one_lane", C.c_int32),
                ("parallel", C.c_int32), ("max_threads", C.c_int32), ("work_per_eval", C.c_double), ("work_one_lane", C.c_double),
                ("rows_n_obs", C.c_int32), ("rows_groups", C.c_int32), ("rows_sweep", C.c_int32)]


EXPORTS = ["amwg_set_pointwise", "amwg_pointwise_n_obs", "amwg_compile_pointwise", "amwg_last_sample_dataset_waic", "amwg_last_sample_dataset_loo", "amwg_last_sample_dataset_hpd", "amwg_last_sample_dataset_autocovariance", "amwg_set_autocovariance", "amwg_autocovariance_info", "amwg_last_sample_dataset_covariance", "amwg_set_covariance", "amwg_covariance_info", "amwg_last_sample_dataset_histogram", "amwg_set_histogram", "amwg_histogram_info", "amwg_sample_summarize","amwg_sample_summarize_async", "amwg_summary_info", "amwg_create_user_datasets", "amwg_compile_user_datasets", "amwg_create_datasets", "amwg_create_datasets_ragged", "amwg_num_datasets", "amwg_dataset_n_obs", "amwg_last_sample_dataset_moments", "amwg_last_sample_dataset_diagnostics", "amwg_last_sample_dataset_quantiles", "amwg_kernel_name", "amwg_summation_order", "amwg_group_gather_draws", "amwg_group_comm_info", "amwg_comm_unique_id", "amwg_comm_create", "amwg_comm_info", "amwg_comm_gather_draws", "amwg_comm_moments", "amwg_comm_destroy", "amwg_code_cache_stats", "amwg_tuning", "amwg_group_moments", "amwg_group_diagnostics", "amwg_group_quantiles", "amwg_last_sample_quantiles", "amwg_fp64_peak", "amwg_set_state", "amwg_last_sample_diagnostics", "amwg_create_user", "amwg_compile_user", "amwg_num_recorded", "amwg_create", "amwg_burn", "amwg_burn_async", "amwg_sample", "amwg_sample_async", "amwg_fetch_draws", "amwg_fetch_draws_slices", "amwg_sample_device", "amwg_set_adapting", "amwg_get_state", "amwg_info", "amwg_chain_diag", "amwg_last_sample_moments", "amwg_sync", "amwg_num_components", "amwg_num_chains", "amwg_launch_info", "amwg_destroy", "amwg_last_error", "amwg_version", "amwg_exp", "amwg_log", "amwg_uniform"]      # include/amwg.h: the product library
SELFTEST_EXPORTS = ["amwg_user_waic_check", "amwg_user_loo_check", "amwg_waic_check", "amwg_loo_check", "amwg_loo_stats", "amwg_hpd_check", "amwg_hpd_limits", "amwg_autocovariance_check", "amwg_covariance_check", "amwg_histogram_check", "amwg_summaries_check","amwg_fold_check","amwg_dataset_quantiles_check", "amwg_prefault_selftest", "amwg_math1", "amwg_math2", "amwg_hypot3", "amwg_log1p", "amwg_expm1", "amwg_two_valued_sum_check", "amwg_two_valued_tables", "amwg_k_valued_sum_check", "amwg_pow", "amwg_ld_host", "amwg_ld_device", "amwg_device_eval", "amwg_stream_check"]      # include/amwg_selftest.h: libamwg_selftest.so only

_lib = None


def lib():
    """Loads libamwg.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libamwg.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
        pd, pi32, pi64, pu64 = C.POINTER(dbl), C.POINTER(i32), C.POINTER(i64), C.POINTER(u64)
        L.amwg_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(ParamDesc), i32, pd, C.POINTER(CompOpt),
                                  C.POINTER(Options), C.POINTER(vp)]
        L.amwg_create_datasets.argtypes = [C.POINTER(ModelDesc), i32, C.POINTER(ParamDesc), i32, pd, C.POINTER(CompOpt),
                                           C.POINTER(Options), C.POINTER(vp)]
        L.amwg_create_datasets_ragged.argtypes = L.amwg_create_datasets.argtypes
        L.amwg_num_datasets.argtypes = [vp]
        L.amwg_dataset_n_obs.argtypes = [vp, pi32]
        L.amwg_last_sample_dataset_moments.argtypes = [vp, pd, pd]
        L.amwg_last_sample_dataset_diagnostics.argtypes = [vp, pd, pd]
        L.amwg_last_sample_dataset_quantiles.argtypes = [vp, pd, i32, pd]
        L.amwg_last_sample_dataset_hpd.argtypes = [vp, pd, i32, pd]
        L.amwg_last_sample_dataset_waic.argtypes = [vp, pd, pi32, pd]
        L.amwg_last_sample_dataset_loo.argtypes = [vp, pd, pi32, pd]
        L.amwg_burn.argtypes = [vp, i64]
        L.amwg_burn_async.argtypes = [vp, i64]
        L.amwg_sample_async.argtypes = [vp, i64, i64]
        L.amwg_fetch_draws.argtypes = [vp, pd, C.c_size_t]
        L.amwg_fetch_draws_slices.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_size_t)]
        L.amwg_sample.argtypes = [vp, i64, i64, pd, C.c_size_t]
        L.amwg_sample_device.argtypes = [vp, i64, i64, vp, C.c_size_t]
        L.amwg_sample_summarize.argtypes = [vp, i64, i64, i64]
        L.amwg_sample_summarize_async.argtypes = [vp, i64, i64, i64]
        L.amwg_summary_info.argtypes = [vp, pi64, pi64, pi64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.amwg_last_sample_dataset_histogram.argtypes = [vp, pd, i32, pu64]
        L.amwg_set_histogram.argtypes = [vp, pd, i32]
        L.amwg_histogram_info.argtypes = [vp, pi32, C.POINTER(C.c_size_t)]
        L.amwg_last_sample_dataset_covariance.argtypes = [vp, pi32, i32, pd]
        L.amwg_set_covariance.argtypes = [vp, pi32, i32]
        L.amwg_covariance_info.argtypes = [vp, pi32, C.POINTER(C.c_size_t)]
        L.amwg_last_sample_dataset_autocovariance.argtypes = [vp, pi32, i32, i32, pd, pd, pd]
        L.amwg_set_autocovariance.argtypes = [vp, pi32, i32, i32]
        L.amwg_autocovariance_info.argtypes = [vp, pi32, pi32, C.POINTER(C.c_size_t)]
        L.amwg_set_adapting.argtypes = [vp, i32]
        L.amwg_get_state.argtypes = [vp, pd, C.c_size_t]
        L.amwg_info.argtypes = [vp, pd, pi32, pi32, pi32, pi64, pi64]
        L.amwg_chain_diag.argtypes = [vp, pu64, pd, pi32]
        L.amwg_last_sample_moments.argtypes = [vp, pd, pd]
        L.amwg_sync.argtypes = [vp]
        L.amwg_num_components.argtypes = [vp]
        L.amwg_num_chains.argtypes = [vp]
        L.amwg_num_chains.restype = i64
        L.amwg_launch_info.argtypes = [vp, pi32, pi32, pi32, pi32, pi32, pd]
        L.amwg_kernel_name.argtypes = [vp]
        L.amwg_summation_order.argtypes = [vp]
        L.amwg_kernel_name.restype = C.c_char_p
        L.amwg_destroy.argtypes = [vp]
        L.amwg_last_error.restype = C.c_char_p
        L.amwg_version.restype = C.c_char_p
        L.amwg_exp.restype = dbl
        L.amwg_exp.argtypes = [dbl]
        L.amwg_log.restype = dbl
        L.amwg_log.argtypes = [dbl]
        L.amwg_uniform.restype = dbl
        L.amwg_uniform.argtypes = [u64, u64, u64]
        L.amwg_compile_user.argtypes = [C.c_char_p, i32, i32, C.c_char_p, C.POINTER(C.c_size_t)]
        L.amwg_code_cache_stats.argtypes = [pi64, pi64, C.c_char_p, C.c_size_t]
        L.amwg_create_user.argtypes = [C.POINTER(UserModel), C.POINTER(ParamDesc), i32, pd, C.POINTER(CompOpt),
                                       C.POINTER(Options), C.POINTER(vp)]
        L.amwg_create_user_datasets.argtypes = [C.POINTER(UserModel), i32, C.POINTER(ParamDesc), i32, pd, C.POINTER(CompOpt), C.POINTER(Options), C.POINTER(vp)]
        L.amwg_compile_user_datasets.argtypes = L.amwg_compile_user.argtypes
        L.amwg_compile_pointwise.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_size_t)]
        L.amwg_set_pointwise.argtypes = [vp, C.c_char_p]
        L.amwg_pointwise_n_obs.argtypes = [vp]
        L.amwg_pointwise_n_obs.restype = i64
        L.amwg_num_recorded.argtypes = [vp]
        L.amwg_set_state.argtypes = [vp, pd, C.c_size_t]
        L.amwg_fp64_peak.argtypes = [i32, pd]
        L.amwg_last_sample_quantiles.argtypes = [vp, pd, i32, pd]
        L.amwg_last_sample_diagnostics.argtypes = [vp, pd, pd]
        pvp = C.POINTER(vp)
        L.amwg_group_moments.argtypes = [pvp, i32, pd, pd]
        L.amwg_group_diagnostics.argtypes = [pvp, i32, pd, pd]
        L.amwg_group_quantiles.argtypes = [pvp, i32, pd, i32, pd]
        L.amwg_group_gather_draws.argtypes = [pvp, i32, i32, vp, pd, C.c_size_t, pi64]
        L.amwg_group_comm_info.argtypes = [pvp, i32, pi32, pi32, i32]
        L.amwg_comm_unique_id.argtypes = [C.c_char_p, C.c_size_t]
        L.amwg_comm_create.argtypes = [C.c_char_p, C.c_size_t, i32, i32, i32, pvp]
        L.amwg_comm_info.argtypes = [vp, pi32, pi32, pi32]
        L.amwg_comm_gather_draws.argtypes = [vp, vp, i32, vp, C.c_size_t, pi64]
        L.amwg_comm_moments.argtypes = [vp, vp, pd, pd]
        L.amwg_comm_destroy.argtypes = [vp]
        _lib = L
    return _lib


_selftest = None


def selftest_lib():
    """libamwg_selftest.so: the product's sources built with -DAMWG_SELFTEST, which adds the entry points of include/amwg_selftest.h (the
    arithmetic building blocks one by one).  Test suite only; the product library does not carry them."""
    global _selftest
    if _selftest is None:
        path = os.path.join(os.path.dirname(LIB_PATH), "libamwg_selftest.so")
        if not os.path.exists(path):
            raise RuntimeError("libamwg_selftest.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(path)
        i32, i64, dbl = C.c_int32, C.c_int64, C.c_double
        pd = C.POINTER(dbl)
        L.amwg_last_error.restype = C.c_char_p
        L.amwg_device_eval.argtypes = [i32, i32, i64, pd, pd, pd, pd]
        L.amwg_two_valued_sum_check.argtypes = [i32, pd, i32, i64, pd, pd, pd, pd, pd]
        L.amwg_k_valued_sum_check.argtypes = [i32, i32, C.POINTER(C.c_uint8), i32, C.POINTER(C.c_uint32), i64, pd, pd, pd, pd]
        L.amwg_two_valued_tables.argtypes = [C.POINTER(C.c_uint8), i32, C.POINTER(C.c_uint32)]
        L.amwg_stream_check.argtypes = [i32, i32, C.c_uint64, C.c_uint64, i64, C.POINTER(C.c_uint64), i64, C.POINTER(C.c_uint8), i64, pd, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.amwg_pow.restype = dbl
        L.amwg_pow.argtypes = [dbl, dbl]
        L.amwg_math1.restype = dbl
        L.amwg_math1.argtypes = [i32, dbl]
        L.amwg_math2.restype = dbl
        L.amwg_math2.argtypes = [i32, dbl, dbl]
        L.amwg_hypot3.restype = dbl
        L.amwg_hypot3.argtypes = [dbl, dbl, dbl]
        for f in ("amwg_log1p", "amwg_expm1"):
            getattr(L, f).restype = dbl
            getattr(L, f).argtypes = [dbl]
        L.amwg_ld_host.restype = dbl
        L.amwg_ld_host.argtypes = [i32, dbl, dbl, dbl, dbl]
        L.amwg_ld_device.argtypes = [i32, i64, pd, pd]
        L.amwg_prefault_selftest.argtypes = [C.c_void_p, C.c_size_t, i32, i32]
        L.amwg_dataset_quantiles_check.argtypes = [i32, pd, i64, i32, i64, i32, pd, i32, pd]
        L.amwg_hpd_check.argtypes = [i32, pd, i64, i32, i64, i32, pd, i32, pd]
        L.amwg_hpd_limits.argtypes = [i32, i64, C.POINTER(i64), C.POINTER(i64)]
        L.amwg_waic_check.argtypes = [i32, pd, i64, i32, i64, i32, C.POINTER(ModelDesc), i64, pd, C.POINTER(i32), pd, pd]
        L.amwg_loo_check.argtypes = [i32, pd, i64, i32, i64, i32, C.POINTER(ModelDesc), i64, pd, C.POINTER(i32), pd, pd]
        L.amwg_user_waic_check.argtypes = [i32, C.POINTER(UserModel), i32, i32, C.c_char_p, pd, i64, i32, i64, i64, pd, C.POINTER(i32), pd, pd]
        L.amwg_user_loo_check.argtypes = L.amwg_user_waic_check.argtypes
        L.amwg_loo_stats.argtypes = [i32, C.POINTER(i32), pd]
        L.amwg_fold_check.argtypes = [i32, pd, i64, i32, i64, i32, i64, pd, pd, pd, pd]
        L.amwg_summaries_check.argtypes = [i32, pd, i64, i32, i64, i32, i64, pd, pd, pd, pd, pd, pd]
        L.amwg_histogram_check.argtypes = [pd, i64, i32, i64, i32, pd, i32, i64, C.POINTER(C.c_uint64), i32]
        L.amwg_covariance_check.argtypes = [pd, i64, i32, i64, i32, C.POINTER(i32), i32, i64, pd, i32]
        L.amwg_autocovariance_check.argtypes = [pd, i64, i32, i64, i32, C.POINTER(i32), i32, i32, i64, pd, pd, pd, i32]
        _selftest = L
    return _selftest


class AmwgError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise AmwgError("amwg error %d: %s" % (rc, lib().amwg_last_error().decode()))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Sampler:
    """Many-chain sampler handle.  `spec` = dict(model, n_obs, data{x[,y,g,G,K]}, params[], P, init[], comp_opts[]) for a
    built-in family, or dict(user={source, arrays[], n_derived, lds_bytes, parallel, max_threads}, params[], P, init[],
    comp_opts[]) for a closure translated by bayes.js_amd/translate.js (amwg_create_user)."""

    def __init__(self, spec, chains, seed, chain_offset=0, device=0, lanes_per_chain=0, block_threads=0,
                 steps_per_launch=0, exact_division=0, group_local=0, full_evaluation=0, test_bound_shift=0, sufficient_statistics=0, ragged=False):
        L = lib()
        keep = []
        specs = None
        # one spec per dataset: amwg_create_datasets, which insists on equal sizes, or with ragged=True amwg_create_datasets_ragged (the parameters, init and
        # stepper options are those of the first)
        if isinstance(spec, (list, tuple)):
            specs = list(spec)
            n_user = sum(1 for q in specs if q.get("user") is not None)
            if not specs or (n_user and n_user != len(specs)):
                raise AmwgError("a list of specs is one built-in family, or one translated closure, on several datasets: it must not be empty or mix the two")
            spec = specs[0]
        user = spec.get("user")

        def user_model(um, user):
            src = user["source"].encode() if isinstance(user["source"], str) else user["source"]
            keep.append(src)
            um.source = src
            arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in user["arrays"]]
            keep.append(arrs)
            um.n_arrays = len(arrs)
            ptrs = (C.POINTER(C.c_double) * max(1, len(arrs)))(*[_dp(a) for a in arrs])
            lens = (C.c_int64 * max(1, len(arrs)))(*[a.size for a in arrs])
            types = (C.c_int32 * max(1, len(arrs)))(*[int(t) for t in user.get("array_types", [0] * len(arrs))])
            keep.extend([ptrs, lens, types])
            um.arrays, um.array_len, um.array_type = ptrs, lens, types
            um.n_derived, um.lds_bytes = int(user.get("n_derived", 0)), int(user.get("lds_bytes", 0))
            um.lds_bytes_one_lane = int(user.get("lds_bytes_one_lane", 0))
            um.parallel, um.max_threads = int(user.get("parallel", 0)), int(user.get("max_threads", 0))
            um.work_per_eval = float(user.get("work_per_eval", 0.0))
            um.work_one_lane = float(user.get("work_one_lane", 0.0))
            um.rows_n_obs, um.rows_groups, um.rows_sweep = int(user.get("rows_n_obs", 0)), int(user.get("rows_groups", 0)), int(user.get("rows_sweep", 0))

        def model_desc(md, q):
            d = q["data"]
            md.model = MODEL_ID[q["model"]]
            md.n_obs = q["n_obs"]
            x = np.ascontiguousarray(d["x"], dtype=np.float64)
            keep.append(x)
            md.x = _dp(x)
            if "y" in d:
                y = np.ascontiguousarray(d["y"], dtype=np.float64)
                keep.append(y)
                md.y = _dp(y)
            if "g" in d:
                g = np.ascontiguousarray(d["g"], dtype=np.int32)
                keep.append(g)
                md.g = g.ctypes.data_as(C.POINTER(C.c_int32))
            md.G = int(q.get("G", 0))
            md.K = int(q.get("K", 0))
            for i, v in enumerate(q.get("hyper") or DEFAULT_HYPER[q["model"]]):
                md.hyper[i] = float(v)

        if specs is not None and user is not None:      # one translated closure on several datasets: amwg_create_user_datasets
            ums = (UserModel * len(specs))()
            for k, q in enumerate(specs):
                user_model(ums[k], q["user"])
        elif specs is not None:
            mds = (ModelDesc * len(specs))()
            for k, q in enumerate(specs):
                model_desc(mds[k], q)
        elif user is None:
            md = ModelDesc()
            model_desc(md, spec)
        else:
            um = UserModel()
            user_model(um, user)
        n = len(spec["params"])
        pa = (ParamDesc * n)()
        TYPE = {"real": 0, "int": 1, "binary": 2}
        for i, p in enumerate(spec["params"]):
            pa[i].type = TYPE[p["type"]]
            pa[i].len, pa[i].top, pa[i].multidim = p["len"], p["top"], p["multidim"]
            pa[i].lower, pa[i].upper = p["lower"], p["upper"]
        P = spec["P"]
        oa = (CompOpt * P)()
        for i, o in enumerate(spec["comp_opts"]):
            oa[i].prop_log_scale = o["prop_log_scale"]
            oa[i].max_adaptation = o["max_adaptation"]
            oa[i].initial_adaptation = o["initial_adaptation"]
            oa[i].target_accept_rate = o["target_accept_rate"]
            oa[i].batch_size = float(o["batch_size"])
            oa[i].is_adapting = int(bool(o["is_adapting"]))
        init = np.ascontiguousarray(spec["init"], dtype=np.float64)
        op = Options()
        op.chains, op.seed, op.chain_offset, op.device = chains, seed, chain_offset, device
        op.lanes_per_chain, op.block_threads, op.steps_per_launch = lanes_per_chain, block_threads, steps_per_launch
        op.exact_division = exact_division
        op.group_local = group_local
        op.full_evaluation = full_evaluation
        op.test_bound_shift = test_bound_shift
        op.sufficient_statistics = sufficient_statistics
        h = C.c_void_p()
        if specs is not None and user is not None:
            _check(L.amwg_create_user_datasets(ums, len(specs), pa, n, _dp(init), oa, C.byref(op), C.byref(h)))
        elif specs is not None:
            create = L.amwg_create_datasets_ragged if ragged else L.amwg_create_datasets
            _check(create(mds, len(specs), pa, n, _dp(init), oa, C.byref(op), C.byref(h)))
        elif user is None:
            _check(L.amwg_create(C.byref(md), pa, n, _dp(init), oa, C.byref(op), C.byref(h)))
        else:
            _check(L.amwg_create_user(C.byref(um), pa, n, _dp(init), oa, C.byref(op), C.byref(h)))
        self.h = h
        self.P = P
        self.PR = L.amwg_num_recorded(h)   # values per draw row: P + derived quantities
        self.C = chains
        self.n_params = n
        self.D = L.amwg_num_datasets(h)      # datasets (1 unless made from a list of specs)
        # options.pointwise: the closure's pointwise text (translate.js), stored on the sampler; compiled at the first waic() / loo()
        terms = spec.get("pointwise") if user is None else user.get("pointwise", spec.get("pointwise"))
        if terms is not None:
            if user is None:
                self.close()
                raise AmwgError("amwg error -1: pointwise: a built-in family needs no flag -- its pointwise terms are known to the library")
            try:
                _check(L.amwg_set_pointwise(h, terms.encode() if isinstance(terms, str) else terms))
            except AmwgError:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None):
            lib().amwg_destroy(self.h)
            self.h = None

    __del__ = close

    def burn(self, n):
        _check(lib().amwg_burn(self.h, n))

    def sample(self, n, thin=1):
        """-> array [kept][P + derived][chains]"""
        kept = -(-n // thin)
        out = np.empty((kept, self.PR, self.C), dtype=np.float64)
        _check(lib().amwg_sample(self.h, n, thin, _dp(out), out.nbytes))
        self._kept = kept
        return out

    def burn_async(self, n):
        _check(lib().amwg_burn_async(self.h, n))

    def sample_async(self, n, thin=1):
        _check(lib().amwg_sample_async(self.h, n, thin))
        self._pending = self._kept = -(-n // thin)

    def fetch_draws(self):
        out = np.empty((self._pending, self.PR, self.C), dtype=np.float64)
        _check(lib().amwg_fetch_draws(self.h, _dp(out), out.nbytes))
        return out

    def fetch_draws_slices(self, slices):
        """slices: [(base, len), ...] -> one array [kept][len][chains] per slice (amwg_fetch_draws_slices)"""
        outs = [np.empty((self._pending, ln, self.C), dtype=np.float64) for _, ln in slices]
        n = len(slices)
        base = (C.c_int32 * max(n, 1))(*[b for b, _ in slices])
        ln = (C.c_int32 * max(n, 1))(*[l for _, l in slices])
        ptrs = (C.POINTER(C.c_double) * max(n, 1))(*[_dp(o) for o in outs])
        sizes = (C.c_size_t * max(n, 1))(*[o.nbytes for o in outs])
        _check(lib().amwg_fetch_draws_slices(self.h, n, base, ln, ptrs, sizes))
        return outs

    def summarize(self, n, thin=1, window_rows=0, covariance=None):
        """The steps of sample_async(n, thin) + sync(), the kept draws folded window by window into per-chain accumulators instead of stored
        (amwg_sample_summarize): moments(), convergence() and their dataset_ forms then answer from those.  -> kept draws
        covariance: shorthand for set_covariance() before the call, which -- like set_histogram() -- arms this AND every later summarize() until it is disarmed:
        True arms the covariance of every recorded value, a list of indices that of those values, False disarms; None (the default) leaves what is armed as it is.
        (mcmc.js takes its options per call instead: a summarize() there without options.covariance disarms.)"""
        if covariance is False:
            self.set_covariance(None)
        elif covariance is not None:
            self.set_covariance(range(self.PR) if covariance is True else covariance)
        _check(lib().amwg_sample_summarize(self.h, n, thin, window_rows))
        self._pending = self._kept = -(-n // thin)
        return self._pending

    def summary_info(self):
        """What the last summarize() held (amwg_summary_info)"""
        r, w, k = C.c_int64(), C.c_int64(), C.c_int64()
        wb, ab = C.c_size_t(), C.c_size_t()
        _check(lib().amwg_summary_info(self.h, C.byref(r), C.byref(w), C.byref(k), C.byref(wb), C.byref(ab)))
        return {"rows": r.value, "window_rows": w.value, "windows": k.value, "window_bytes": wb.value, "accumulator_bytes": ab.value}

    def set_histogram(self, edges):
        """Arms a histogram for every later summarize() (amwg_set_histogram): edges [bins + 1] for all recorded values, or [P + derived][bins + 1];
        None disarms.  dataset_histogram() returns the counts after the call."""
        if edges is None:
            _check(lib().amwg_set_histogram(self.h, None, 0))
            return
        e = _edges_per_value(edges, self.PR)
        _check(lib().amwg_set_histogram(self.h, _dp(e), e.shape[1] - 1))

    def histogram_info(self):
        """{"bins": the armed number of bins (0: none), "bytes": the device bytes of its edges and counts} (amwg_histogram_info)"""
        b, n = C.c_int32(), C.c_size_t()
        _check(lib().amwg_histogram_info(self.h, C.byref(b), C.byref(n)))
        return {"bins": b.value, "bytes": n.value}

    def dataset_histogram(self, edges=None):
        """-> uint64 array [datasets][P + derived][bins + 3] (the bins, then under, over, nan) over the last sample call, counted on the device by the rule
        np.searchsorted(edges, x, side="right") - 1 (amwg_last_sample_dataset_histogram).  After sample*(): under any `edges` ([bins + 1] or
        [P + derived][bins + 1]).  After summarize(): edges=None, the counts under the edges of set_histogram()."""
        if edges is None:
            bins = self.histogram_info()["bins"]
            out = np.zeros((self.D, self.PR, max(bins, 1) + 3), dtype=np.uint64)
            _check(lib().amwg_last_sample_dataset_histogram(self.h, None, bins, out.ctypes.data_as(C.POINTER(C.c_uint64))))
            return out
        e = _edges_per_value(edges, self.PR)
        out = np.zeros((self.D, self.PR, e.shape[1] + 2), dtype=np.uint64)
        _check(lib().amwg_last_sample_dataset_histogram(self.h, _dp(e), e.shape[1] - 1, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def _summarised(self):
        """was the last sample call a summarising one?  The library knows (amwg_summary_info succeeds only then); a refusal here is the answer, not an error."""
        return lib().amwg_summary_info(self.h, None, None, None, None, None) == 0

    def set_covariance(self, values):
        """Arms the covariance of the recorded values `values` (distinct indices; components, then derived quantities) for every later summarize()
        (amwg_set_covariance); None disarms.  dataset_covariance() returns the matrices after the call."""
        if values is None:
            _check(lib().amwg_set_covariance(self.h, None, 0))
            return
        v = _value_list(values)
        _check(lib().amwg_set_covariance(self.h, v.ctypes.data_as(C.POINTER(C.c_int32)), v.size))

    def covariance_info(self):
        """{"n_values": the armed number of values (0: none), "bytes": the device bytes of its co-moments and list} (amwg_covariance_info)"""
        k, n = C.c_int32(), C.c_size_t()
        _check(lib().amwg_covariance_info(self.h, C.byref(k), C.byref(n)))
        return {"n_values": k.value, "bytes": n.value}

    def dataset_covariance(self, values=None):
        """-> array [datasets][K][K]: per dataset the covariance matrix (n - 1 denominator over chains x kept draws) of the recorded values `values`, in
        their order, formed on the device (amwg_last_sample_dataset_covariance).  After sample*(): any distinct `values` (None: every recorded value).
        After summarize(): values=None, the matrix over the values of set_covariance().  correlation() turns it into correlations."""
        if values is None and self._summarised():
            K = self.covariance_info()["n_values"]
            out = np.zeros((self.D, max(K, 1), max(K, 1)))
            _check(lib().amwg_last_sample_dataset_covariance(self.h, None, max(K, 1), _dp(out)))
            return out
        v = _value_list(range(self.PR) if values is None else values)
        out = np.zeros((self.D, v.size, v.size))
        _check(lib().amwg_last_sample_dataset_covariance(self.h, v.ctypes.data_as(C.POINTER(C.c_int32)), v.size, _dp(out)))
        return out

    def set_autocovariance(self, values, max_lag=0):
        """Arms the autocovariance at lags 0 .. max_lag of the recorded values `values` (distinct indices) for every later summarize() (amwg_set_autocovariance);
        None disarms.  A summarize() that would keep <= max_lag draws is then refused before it runs.  dataset_autocovariance() returns the result after the call."""
        if values is None:
            _check(lib().amwg_set_autocovariance(self.h, None, 0, 0))
            return
        v = _value_list(values)
        _check(lib().amwg_set_autocovariance(self.h, v.ctypes.data_as(C.POINTER(C.c_int32)), v.size, max_lag))

    def autocovariance_info(self):
        """{"n_values": the armed number of values (0: none), "max_lag", "bytes": the device bytes of its lag sums, rows and list} (amwg_autocovariance_info)"""
        k, lag, n = C.c_int32(), C.c_int32(), C.c_size_t()
        _check(lib().amwg_autocovariance_info(self.h, C.byref(k), C.byref(lag), C.byref(n)))
        return {"n_values": k.value, "max_lag": lag.value, "bytes": n.value}

    def dataset_autocovariance(self, values=None, max_lag=None):
        """-> (acov [datasets][K][max_lag + 1], mean [datasets][K], between [datasets][K]): per dataset and recorded value of `values`, in their order, the
        autocovariance at lags 0 .. max_lag averaged over the dataset's chains (1 / n denominator per chain), the mean and the variance of the chain means
        (n - 1 denominator; 0 for one chain), formed on the device (amwg_last_sample_dataset_autocovariance).  After sample*(): any distinct `values` (None: every
        recorded value) and max_lag (None: min(100, kept draws - 1)).  After summarize(): both None, what set_autocovariance() armed.
        autocorrelation_ess() turns one row of it into rho, tau and an effective sample size."""
        if values is None and max_lag is None and self._summarised():
            info = self.autocovariance_info()
            K, lag = max(info["n_values"], 1), max(info["max_lag"], 1)
            ptr = None
        else:
            v = _value_list(range(self.PR) if values is None else values)
            K, lag = v.size, (min(100, getattr(self, "_kept", 0) - 1) if max_lag is None else int(max_lag))
            ptr = v.ctypes.data_as(C.POINTER(C.c_int32))
        acov, mean, between = np.zeros((self.D, K, max(lag, 0) + 1)), np.zeros((self.D, K)), np.zeros((self.D, K))
        _check(lib().amwg_last_sample_dataset_autocovariance(self.h, ptr, K, lag, _dp(acov), _dp(mean), _dp(between)))
        return acov, mean, between

    def sample_device(self, n, thin, dev_ptr, nbytes):
        _check(lib().amwg_sample_device(self.h, n, thin, C.c_void_p(dev_ptr), nbytes))

    def sync(self):
        _check(lib().amwg_sync(self.h))

    def set_adapting(self, flag):
        _check(lib().amwg_set_adapting(self.h, int(bool(flag))))

    def state(self):
        out = np.empty((self.P, self.C), dtype=np.float64)
        _check(lib().amwg_get_state(self.h, _dp(out), out.nbytes))
        return out

    def info(self):
        P, Cn = self.P, self.C
        pls = np.empty((P, Cn))
        ac, it, bc = (np.empty((P, Cn), dtype=np.int32) for _ in range(3))
        acc, inb = (np.empty((P, Cn), dtype=np.int64) for _ in range(2))
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        _check(lib().amwg_info(self.h, _dp(pls), i32(ac), i32(it), i32(bc), i64(acc), i64(inb)))
        return {"prop_log_scale": pls, "acceptance_count": ac, "iterations_since_adaption": it, "batch_count": bc,
                "accepts": acc, "inbounds": inb}

    def diag(self):
        un = np.empty(self.C, dtype=np.uint64)
        lp = np.empty(self.C)
        order = np.empty((self.C, self.n_params), dtype=np.int32)
        _check(lib().amwg_chain_diag(self.h, un.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(lp),
                                     order.ctypes.data_as(C.POINTER(C.c_int32))))
        return {"uniforms": un, "log_post": lp, "named_order": order}

    def moments(self):
        m, s = np.empty(self.PR), np.empty(self.PR)
        _check(lib().amwg_last_sample_moments(self.h, _dp(m), _dp(s)))
        return m, s

    def dataset_n_obs(self):
        """-> list of the datasets' sizes (amwg_dataset_n_obs); an ordinary sampler: its one size"""
        out = np.zeros(max(1, self.D), dtype=np.int32)
        _check(lib().amwg_dataset_n_obs(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out.tolist()

    def pointwise_n_obs(self):
        """-> the observations per dataset of a closure whose pointwise text is set (amwg_pointwise_n_obs); 0 otherwise"""
        return int(lib().amwg_pointwise_n_obs(self.h))

    def _n_max(self):
        return max(self.dataset_n_obs() + [self.pointwise_n_obs()])

    def dataset_moments(self):
        """-> mean, sd, arrays [datasets][P + derived]: moments() per dataset (amwg_last_sample_dataset_moments)"""
        m, s = np.empty((self.D, self.PR)), np.empty((self.D, self.PR))
        _check(lib().amwg_last_sample_dataset_moments(self.h, _dp(m), _dp(s)))
        return m, s

    def dataset_convergence(self):
        """-> rhat, ess, arrays [datasets][P + derived]: convergence() per dataset (amwg_last_sample_dataset_diagnostics)"""
        r, e = np.empty((self.D, self.PR)), np.empty((self.D, self.PR))
        _check(lib().amwg_last_sample_dataset_diagnostics(self.h, _dp(r), _dp(e)))
        return r, e

    def dataset_quantiles(self, probs):
        """-> array [datasets][P + derived][len(probs)]: quantiles() per dataset, a radix select on the device (amwg_last_sample_dataset_quantiles)"""
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        out = np.empty((self.D, self.PR, pr.size))
        _check(lib().amwg_last_sample_dataset_quantiles(self.h, _dp(pr), pr.size, _dp(out)))
        return out

    def dataset_hpd(self, probs):
        """-> array [datasets][P + derived][len(probs)][2]: the highest-density interval (lower, upper) per dataset, value and probability, by the rule of
        include/amwg.h -- the shortest interval spanning floor(p N) + 1 sorted draws -- on the device (amwg_last_sample_dataset_hpd)"""
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        out = np.empty((self.D, self.PR, pr.size, 2))
        _check(lib().amwg_last_sample_dataset_hpd(self.h, _dp(pr), pr.size, _dp(out)))
        return out

    def hpd(self, probs):
        """-> array [P + derived][len(probs)][2]: dataset_hpd() of an ordinary sampler; a dataset sampler refuses the pooled question"""
        if self.D > 1:
            raise AmwgError("amwg error -1: hpd: this sampler runs %d datasets, a posterior each: pooled summaries are refused -- use amwg_last_sample_dataset_hpd "
                            "(dataset_hpd)" % self.D)      # (the words of amwg_refuse_pooled; the library has no pooled call to ask)
        return self.dataset_hpd(probs)[0]

    def dataset_waic(self, pointwise=False):
        """-> dict(summary [datasets][4] = elpd_waic, se, p_waic, lppd; high [datasets] = observations with p_i > 0.4; with pointwise=True also
        pointwise [datasets][n_max][2] = lppd_i, p_i, NaN beyond a dataset's n_obs): WAIC per dataset by the rule of include/amwg.h, the families' pointwise
        terms over the stored draws on the device (amwg_last_sample_dataset_waic)"""
        summary, high = np.empty((self.D, 4)), np.zeros(self.D, dtype=np.int32)
        pw = np.empty((self.D, self._n_max(), 2)) if pointwise else None
        _check(lib().amwg_last_sample_dataset_waic(self.h, _dp(summary), high.ctypes.data_as(C.POINTER(C.c_int32)), _dp(pw) if pointwise else None))
        out = {"summary": summary, "high": high}
        if pointwise:
            out["pointwise"] = pw
        return out

    def waic(self, pointwise=False):
        """-> dict(elpd_waic, se, p_waic, lppd, high[, pointwise [n_obs][2]]): dataset_waic() of an ordinary sampler; a dataset sampler refuses the pooled question"""
        if self.D > 1:
            raise AmwgError("amwg error -1: waic: this sampler runs %d datasets, a posterior each: pooled summaries are refused -- use amwg_last_sample_dataset_waic "
                            "(dataset_waic)" % self.D)      # (the words of amwg_refuse_pooled; the library has no pooled call to ask)
        r = self.dataset_waic(pointwise)
        out = dict(zip(("elpd_waic", "se", "p_waic", "lppd"), r["summary"][0].tolist()), high=int(r["high"][0]))
        if pointwise:
            out["pointwise"] = r["pointwise"][0]
        return out

    def dataset_loo(self, pointwise=False):
        """-> dict(summary [datasets][4] = elpd_loo, se, p_loo, lppd; high [datasets] = observations with khat_i > 0.7; with pointwise=True also
        pointwise [datasets][n_max][3] = elpd_loo_i, lppd_i, khat_i, NaN beyond a dataset's n_obs): PSIS-LOO per dataset by the rule of include/amwg.h, the
        families' pointwise terms over the stored draws on the device (amwg_last_sample_dataset_loo)"""
        summary, high = np.empty((self.D, 4)), np.zeros(self.D, dtype=np.int32)
        pw = np.empty((self.D, self._n_max(), 3)) if pointwise else None
        _check(lib().amwg_last_sample_dataset_loo(self.h, _dp(summary), high.ctypes.data_as(C.POINTER(C.c_int32)), _dp(pw) if pointwise else None))
        out = {"summary": summary, "high": high}
        if pointwise:
            out["pointwise"] = pw
        return out

    def loo(self, pointwise=False):
        """-> dict(elpd_loo, se, p_loo, lppd, high[, pointwise [n_obs][3]]): dataset_loo() of an ordinary sampler; a dataset sampler refuses the pooled question"""
        if self.D > 1:
            raise AmwgError("amwg error -1: loo: this sampler runs %d datasets, a posterior each: pooled summaries are refused -- use amwg_last_sample_dataset_loo "
                            "(dataset_loo)" % self.D)      # (the words of amwg_refuse_pooled; the library has no pooled call to ask)
        r = self.dataset_loo(pointwise)
        out = dict(zip(("elpd_loo", "se", "p_loo", "lppd"), r["summary"][0].tolist()), high=int(r["high"][0]))
        if pointwise:
            out["pointwise"] = r["pointwise"][0]
        return out

    def set_state(self, state):
        st = np.ascontiguousarray(state, dtype=np.float64)
        assert st.shape == (self.P, self.C)
        _check(lib().amwg_set_state(self.h, _dp(st), st.nbytes))

    def convergence(self):
        r, e = np.empty(self.PR), np.empty(self.PR)
        _check(lib().amwg_last_sample_diagnostics(self.h, _dp(r), _dp(e)))
        return r, e

    def quantiles(self, probs):
        """-> array [P + derived][len(probs)] over all chains x kept draws of the last sample()"""
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        out = np.empty((self.PR, pr.size))
        _check(lib().amwg_last_sample_quantiles(self.h, _dp(pr), pr.size, _dp(out)))
        return out

    def tuning(self):
        """AMWG_LANES_AUTOTUNE (lanes_per_chain=-2): [(lanes per chain, ms of the timing run)] of every candidate timed at construction"""
        L = lib()
        L.amwg_tuning.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32]
        lanes, ms = (C.c_int32 * 16)(), (C.c_double * 16)()
        n = L.amwg_tuning(self.h, lanes, ms, 16)
        return [(lanes[i], ms[i]) for i in range(min(n, 16))]

    def launch_info(self):
        v = [C.c_int32() for _ in range(5)]
        ms = C.c_double()
        _check(lib().amwg_launch_info(self.h, *[C.byref(x) for x in v], C.byref(ms)))
        return {"lanes_per_chain": v[0].value, "block_threads": v[1].value, "grid_blocks": v[2].value,
                "lds_bytes": v[3].value, "n_launches": v[4].value, "kernel_ms": ms.value, "kernel": (lib().amwg_kernel_name(self.h) or b"").decode(),
                "summation_order": lib().amwg_summation_order(self.h), "datasets": lib().amwg_num_datasets(self.h)}


def _edges_per_value(edges, PR):
    """edges [bins + 1] (for every recorded value) or [PR][bins + 1] -> contiguous float64 [PR][bins + 1]"""
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1:
        e = np.broadcast_to(e, (PR, e.size))
    if e.ndim != 2 or e.shape[0] != PR or e.shape[1] < 1:
        raise AmwgError("edges must be [bins + 1] or [%d recorded values][bins + 1], got shape %s" % (PR, e.shape))
    return np.ascontiguousarray(e)


def _value_list(values):
    v = np.ascontiguousarray(np.asarray(list(values), dtype=np.int64).reshape(-1))
    if v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 31):
        raise AmwgError("a list of recorded values holds an index beyond 32 bits")
    return np.ascontiguousarray(v.astype(np.int32))


def covariance_check(draws, D, values, window_rows=0, device=0):
    """libamwg_selftest.so: the kernels of Sampler.dataset_covariance / set_covariance on any array draws [rows][PR][C], D datasets of C / D columns each, over the
    recorded values `values`; window_rows = 0: the stored path, > 0: folded in windows of that many rows through the fold + co-moment sequence of summarize()
    -> array [D][K][K] (amwg_covariance_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    rows, PR, Cn = dr.shape
    v = _value_list(values)
    out = np.zeros((D, max(v.size, 1), max(v.size, 1)))
    L = selftest_lib()
    if L.amwg_covariance_check(_dp(dr), rows, PR, Cn, D, v.ctypes.data_as(C.POINTER(C.c_int32)), v.size, window_rows, _dp(out), device) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return out


def autocovariance_check(draws, D, values, max_lag, window_rows=0, device=0):
    """libamwg_selftest.so: the kernels of Sampler.dataset_autocovariance / set_autocovariance on any array draws [rows][PR][C], D datasets of C / D columns each,
    over the recorded values `values` at lags 0 .. max_lag; window_rows = 0: the stored path, > 0: in windows of that many rows through the lag-sum and carry
    kernels as summarize() enqueues them -> (acov [D][K][max_lag + 1], mean [D][K], between [D][K]) (amwg_autocovariance_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    rows, PR, Cn = dr.shape
    v = _value_list(values)
    K = max(v.size, 1)
    acov, mean, between = np.zeros((D, K, max(int(max_lag), 0) + 1)), np.zeros((D, K)), np.zeros((D, K))
    L = selftest_lib()
    if L.amwg_autocovariance_check(_dp(dr), rows, PR, Cn, D, v.ctypes.data_as(C.POINTER(C.c_int32)), v.size, max_lag, window_rows, _dp(acov), _dp(mean), _dp(between), device) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return acov, mean, between


def autocorrelation_ess(acov, between, rows, chains):
    """One (dataset, value) of dataset_autocovariance() -> {"rho", "tau", "ess", "truncated", "lags_used"}: the autocorrelation, the integrated autocorrelation
    time and the effective sample size of `chains` chains of `rows` kept draws each, by Geyer's initial monotone sequence (BDA3 section 11.5; Stan's ess without rank
    normalisation).  Host arithmetic; no device call.  acov [L + 1].
        var_plus = acov_0 + (chains > 1 ? between : 0);  rho_l = 1 - (n / (n - 1)) (acov_0 - acov_l) / var_plus, rho_0 = 1 exactly;
        P_k = rho_2k + rho_(2k+1), k = 0 .. floor((L + 1) / 2) - 1; the sum stops before the first P_k < 0 (truncated = True) and each kept P_k is replaced by
        min(P_k, P_(k-1));  tau = -1 + 2 sum P_k;  ess = chains rows / tau;  lags_used = twice the number of pairs kept.
    truncated = False: no negative pair was reached within max_lag -- the sum is still growing, `ess` is an UPPER bound, and the caller should ask for more lags.
    var_plus = 0 or not finite: rho (except rho_0), tau and ess are NaN."""
    g = np.asarray(acov, dtype=np.float64).reshape(-1)
    n, M = float(rows), float(chains)
    rho = np.full(g.size, np.nan)
    rho[0] = 1.0
    var_plus = g[0] + (float(between) if chains > 1 else 0.0)
    if not (math.isfinite(var_plus) and var_plus != 0.0):
        return {"rho": rho, "tau": math.nan, "ess": math.nan, "truncated": False, "lags_used": 0}
    for l in range(1, g.size):
        rho[l] = 1.0 - (n / (n - 1.0)) * (g[0] - g[l]) / var_plus
    total, prev, used, truncated = 0.0, math.inf, 0, False
    for k in range(g.size // 2):
        p = rho[2 * k] + rho[2 * k + 1]
        if not p >= 0.0:      # (a NaN stops the sum too)
            truncated = True
            break
        prev = min(p, prev)
        total += prev
        used += 1
    tau = -1.0 + 2.0 * total
    return {"rho": rho, "tau": tau, "ess": float(np.float64(M * n) / np.float64(tau)) if tau != 0.0 else math.inf, "truncated": truncated, "lags_used": 2 * used}


def correlation(cov):
    """cov [..., K, K] -> correlations of the same shape: cov_ij / (sd_i sd_j) with sd = sqrt(cov_ii), clamped to [-1, 1]; the diagonal is 1; NaN where a
    variance is 0 or not finite (and where the covariance is NaN).  Host arithmetic; no device call."""
    c = np.asarray(cov, dtype=np.float64)
    if c.ndim < 2 or c.shape[-1] != c.shape[-2]:
        raise AmwgError("correlation: square matrices [..., K, K], got shape %s" % (c.shape,))
    var = np.diagonal(c, axis1=-2, axis2=-1)
    ok = np.isfinite(var) & (var > 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sd = np.sqrt(np.where(ok, var, np.nan))
        r = c / (sd[..., :, None] * sd[..., None, :])
        r = np.where(np.isnan(r), np.nan, np.clip(r, -1.0, 1.0))
    k = np.arange(c.shape[-1])
    r[..., k, k] = np.where(ok, 1.0, np.nan)
    return r


def histogram_check(draws, D, edges, window_rows=0, counts=None, device=0):
    """libamwg_selftest.so: the kernel of Sampler.dataset_histogram / set_histogram on any array draws [rows][PR][C], D datasets of C / D columns each, under
    edges [bins + 1] or [PR][bins + 1], in windows of window_rows rows (0: all at once); the kernel ADDS to `counts` (default: zeros)
    -> uint64 array [D][PR][bins + 3]: the bins, then under, over, nan (amwg_histogram_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    rows, PR, Cn = dr.shape
    e = _edges_per_value(edges, PR)
    bins = e.shape[1] - 1
    out = np.zeros((D, PR, bins + 3), dtype=np.uint64) if counts is None else np.array(counts, dtype=np.uint64).reshape(D, PR, bins + 3)
    L = selftest_lib()
    if L.amwg_histogram_check(_dp(dr), rows, PR, Cn, D, _dp(e), bins, window_rows, out.ctypes.data_as(C.POINTER(C.c_uint64)), device) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return out


def interval_brackets(counts, edges, probs):
    """For one cell of counts [bins + 3] (the bins, then under, over, nan) under edges [bins + 1]: per probability q the bracket [lo, hi] that contains the value
    quantiles() returns for q over the counted draws (R's type 7: h = (n - 1) q, an interpolation between the order statistics of ranks floor(h) and
    min(floor(h) + 1, n - 1)): lo = the left edge of the bin that holds the first rank (-inf in `under`, edges[bins] in `over`), hi = the right edge of the bin
    that holds the second (+inf in `over`, edges[0] in `under`).  NaN, NaN when a NaN was counted, nothing was counted, or q is outside [0, 1].
    Host arithmetic on integers; no device call.  -> array [len(probs)][2]"""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    bins = e.size - 1
    if bins < 1 or len(c) != bins + 3:
        raise AmwgError("interval_brackets: counts [bins + 3] under edges [bins + 1], got %d counts and %d edges" % (len(c), e.size))
    under, over, nan = c[bins], c[bins + 1], c[bins + 2]
    n = sum(c[:bins]) + under + over
    cum = [under]      # cum[k]: the values below edges[k]; rank r lies in `under` when r < cum[0], in bin i when cum[i] <= r < cum[i + 1], else in `over`
    for v in c[:bins]:
        cum.append(cum[-1] + v)
    out = np.full((len(probs), 2), np.nan)
    for k, q in enumerate(probs):
        q = float(q)
        if nan > 0 or n == 0 or not (0.0 <= q <= 1.0):
            continue
        h = float(n - 1) * q
        r0 = int(np.floor(h))
        r1 = min(r0 + 1, n - 1)
        b0, b1 = bisect.bisect_right(cum, r0) - 1, bisect.bisect_right(cum, r1) - 1      # -1: under, bins: over, else the bin
        out[k, 0] = -np.inf if b0 < 0 else e[b0]      # (e[bins] when the rank lies in `over`)
        out[k, 1] = np.inf if b1 >= bins else e[b1 + 1]      # (e[0] when it lies in `under`)
    return out


def dataset_quantiles_check(draws, D, probs, device=0):
    """libamwg_selftest.so: the kernel of Sampler.dataset_quantiles on any array draws [rows][PR][C], D datasets of C / D columns each
    -> array [D][PR][len(probs)] (amwg_dataset_quantiles_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    rows, PR, Cn = dr.shape
    out = np.empty((D, PR, pr.size))
    L = selftest_lib()
    if L.amwg_dataset_quantiles_check(device, _dp(dr), rows, PR, Cn, D, _dp(pr), pr.size, _dp(out)) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return out


def hpd_check(draws, D, probs, device=0):
    """libamwg_selftest.so: the kernels of Sampler.dataset_hpd on any array draws [rows][PR][C], D datasets of C / D columns each
    -> array [D][PR][len(probs)][2] (amwg_hpd_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    rows, PR, Cn = dr.shape
    out = np.empty((D, PR, pr.size, 2))
    L = selftest_lib()
    if L.amwg_hpd_check(device, _dp(dr), rows, PR, Cn, D, _dp(pr), pr.size, _dp(out)) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return out


def waic_totals(pointwise, n_obs):
    """The finish of amwg_last_sample_dataset_waic restated (include/amwg.h): pointwise [n_max][2] = lppd_i, p_i of ONE dataset with n_obs observations
    -> (summary [4] = elpd_waic, se, p_waic, lppd; high).  Running sums from 0.0 in index order, one IEEE operation each: the bytes of the library's."""
    pw = np.asarray(pointwise, dtype=np.float64)
    n = int(n_obs)
    lppd = p = elpd = np.float64(0.0)
    high = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            lppd = lppd + pw[i, 0]
            p = p + pw[i, 1]
            elpd = elpd + (pw[i, 0] - pw[i, 1])
            high += 1 if pw[i, 1] > 0.4 else 0
        centre = elpd / np.float64(n)
        ss = np.float64(0.0)
        for i in range(n):
            e = (pw[i, 0] - pw[i, 1]) - centre
            ss = ss + e * e
        se = np.float64(np.nan) if n == 1 else np.sqrt(np.float64(n) * ss / np.float64(n - 1))
    return np.array([elpd, se, p, lppd]), high


def _model_descs(specs):
    """specs -> (the ModelDesc array of the check calls, the arrays it points into: keep them alive over the call)"""
    D = len(specs)
    keep = []
    mds = (ModelDesc * max(1, D))()
    for k, q in enumerate(specs):
        d = q["data"]
        mds[k].model, mds[k].n_obs = MODEL_ID[q["model"]], int(q["n_obs"])
        x = np.ascontiguousarray(d["x"], dtype=np.float64)
        keep.append(x)
        mds[k].x = _dp(x)
        if "y" in d:
            y = np.ascontiguousarray(d["y"], dtype=np.float64)
            keep.append(y)
            mds[k].y = _dp(y)
        if "g" in d:
            g = np.ascontiguousarray(d["g"], dtype=np.int32)
            keep.append(g)
            mds[k].g = g.ctypes.data_as(C.POINTER(C.c_int32))
        mds[k].G, mds[k].K = int(q.get("G", 0)), int(q.get("K", 0))
    return mds, keep


def waic_check(draws, specs, pointwise=True, loglik=False, scratch_bytes=0, device=0):
    """libamwg_selftest.so: the kernels of Sampler.dataset_waic on any array draws [rows][PR][C] and the data of `specs`, one dict(model, n_obs, data{x[,y,g]}[, G, K])
    per dataset (one family; ragged sizes allowed), C / len(specs) columns each -> dict(summary [D][4], high [D][, pointwise [D][n_max][2]][, loglik [D][S][n_max],
    the terms themselves in draw order s = row * (C / D) + chain]) (amwg_waic_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    if dr.ndim != 3:
        raise AmwgError("amwg error: waic_check: draws must be [rows][PR][C]")
    rows, PR, Cn = dr.shape
    D = len(specs)
    mds, keep = _model_descs(specs)
    n_max = max([int(q["n_obs"]) for q in specs] + [1])
    S = rows * (Cn // D) if D and Cn % D == 0 else 0
    summary, high = np.empty((max(1, D), 4)), np.zeros(max(1, D), dtype=np.int32)
    pw = np.empty((max(1, D), n_max, 2)) if pointwise else None
    ll = np.empty((max(1, D), S, n_max)) if loglik and S * n_max * max(1, D) <= (1 << 24) else None
    if loglik and ll is None:
        ll = np.empty(1)      # (refused by the library before it is written: more than 2^24 doubles)
    L = selftest_lib()
    if L.amwg_waic_check(device, _dp(dr), rows, PR, Cn, D, mds, scratch_bytes, _dp(summary), high.ctypes.data_as(C.POINTER(C.c_int32)),
                         _dp(pw) if pointwise else None, _dp(ll) if loglik else None) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    out = {"summary": summary, "high": high}
    if pointwise:
        out["pointwise"] = pw
    if loglik:
        out["loglik"] = ll
    return out


def _user_models(users):
    """users: one dict(source, arrays[, array_types, ...]) per dataset -> (the UserModel array of the check calls, what it points into)"""
    keep = []
    ums = (UserModel * max(1, len(users)))()
    for k, user in enumerate(users):
        src = user["source"].encode() if isinstance(user["source"], str) else user["source"]
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in user["arrays"]]
        ptrs = (C.POINTER(C.c_double) * max(1, len(arrs)))(*[_dp(a) for a in arrs])
        lens = (C.c_int64 * max(1, len(arrs)))(*[a.size for a in arrs])
        types = (C.c_int32 * max(1, len(arrs)))(*[int(t) for t in user.get("array_types", [0] * len(arrs))])
        keep.extend([src, arrs, ptrs, lens, types])
        ums[k].source, ums[k].n_arrays, ums[k].arrays, ums[k].array_len, ums[k].array_type = src, len(arrs), ptrs, lens, types
    return ums, keep


def _user_check(loo, draws, users, terms, P, n_obs, pointwise, extra, scratch_bytes, device):
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    if dr.ndim != 3:
        raise AmwgError("amwg error: user_%s_check: draws must be [rows][PR][C]" % ("loo" if loo else "waic"))
    rows, PR, Cn = dr.shape
    D = len(users)
    ums, keep = _user_models(users)
    n_max = max(1, int(n_obs))
    S = rows * (Cn // D) if D and Cn % D == 0 else 0
    width = (loo_tail_len(S) + 1) if loo else S
    summary, high = np.empty((max(1, D), 4)), np.zeros(max(1, D), dtype=np.int32)
    pw = np.empty((max(1, D), n_max, 3 if loo else 2)) if pointwise else None
    ex = None
    if extra:
        ex = (np.empty((max(1, D), n_max, width)) if loo else np.empty((max(1, D), S, n_max))) if width * n_max * max(1, D) <= (1 << 24) else np.empty(1)
    L = selftest_lib()
    call = L.amwg_user_loo_check if loo else L.amwg_user_waic_check
    if call(device, ums, D, int(P), terms.encode() if isinstance(terms, str) else terms, _dp(dr), rows, PR, Cn, scratch_bytes, _dp(summary), high.ctypes.data_as(C.POINTER(C.c_int32)),
            _dp(pw) if pointwise else None, _dp(ex) if extra else None) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    out = {"summary": summary, "high": high}
    if pointwise:
        out["pointwise"] = pw
    if extra:
        out["tails" if loo else "loglik"] = ex
    return out


def user_waic_check(draws, users, terms, P, n_obs, pointwise=True, loglik=False, scratch_bytes=0, device=0):
    """libamwg_selftest.so: waic_check for a translated closure -- users: one dict(source, arrays[, array_types]) per dataset (one source), terms: the pointwise
    text of translate.js (options.pointwise), P the components of the state, n_obs its kTermN -> what waic_check returns (amwg_user_waic_check)"""
    return _user_check(False, draws, users, terms, P, n_obs, pointwise, loglik, scratch_bytes, device)


def user_loo_check(draws, users, terms, P, n_obs, pointwise=True, tails=False, scratch_bytes=0, device=0):
    """libamwg_selftest.so: loo_check for a translated closure, as user_waic_check (amwg_user_loo_check)"""
    return _user_check(True, draws, users, terms, P, n_obs, pointwise, tails, scratch_bytes, device)


def compile_pointwise(source, terms, arch="gfx950"):
    """-> bytes of the code object: hiprtc compilation of a closure's pointwise program without a device (amwg_compile_pointwise)"""
    n = C.c_size_t(0)
    _check(lib().amwg_compile_pointwise(source.encode() if isinstance(source, str) else source, terms.encode() if isinstance(terms, str) else terms, arch.encode(), C.byref(n)))
    return int(n.value)


def loo_tail_len(S):
    """M = min(S // 5, the smallest m3 with m3^2 >= 9 S), in integers: the tail length of amwg_last_sample_dataset_loo (include/amwg.h)"""
    import math
    S = int(S)
    m3 = math.isqrt(9 * S)
    if m3 * m3 < 9 * S:
        m3 += 1
    return min(S // 5, m3)


def loo_totals(pointwise, n_obs):
    """The finish of amwg_last_sample_dataset_loo restated (include/amwg.h): pointwise [n_max][3] = elpd_loo_i, lppd_i, khat_i of ONE dataset with n_obs
    observations -> (summary [4] = elpd_loo, se, p_loo, lppd; high).  Running sums from 0.0 in index order, one IEEE operation each: the bytes of the library's."""
    pw = np.asarray(pointwise, dtype=np.float64)
    n = int(n_obs)
    elpd = lppd = np.float64(0.0)
    high = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            elpd = elpd + pw[i, 0]
            lppd = lppd + pw[i, 1]
            high += 1 if pw[i, 2] > 0.7 else 0
        centre = elpd / np.float64(n)
        ss = np.float64(0.0)
        for i in range(n):
            e = pw[i, 0] - centre
            ss = ss + e * e
        se = np.float64(np.nan) if n == 1 else np.sqrt(np.float64(n) * ss / np.float64(n - 1))
        return np.array([elpd, se, lppd - elpd, lppd]), high


def loo_check(draws, specs, pointwise=True, tails=False, scratch_bytes=0, device=0):
    """libamwg_selftest.so: the kernels of Sampler.dataset_loo on any array draws [rows][PR][C] and the data of `specs` (as waic_check takes them) ->
    dict(summary [D][4], high [D][, pointwise [D][n_max][3]][, tails [D][n_max][M + 1], the sorted smallest terms the fit read]) (amwg_loo_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    if dr.ndim != 3:
        raise AmwgError("amwg error: loo_check: draws must be [rows][PR][C]")
    rows, PR, Cn = dr.shape
    D = len(specs)
    mds, keep = _model_descs(specs)
    n_max = max([int(q["n_obs"]) for q in specs] + [1])
    S = rows * (Cn // D) if D and Cn % D == 0 else 0
    M = loo_tail_len(S)
    summary, high = np.empty((max(1, D), 4)), np.zeros(max(1, D), dtype=np.int32)
    pw = np.empty((max(1, D), n_max, 3)) if pointwise else None
    tl = np.empty((max(1, D), n_max, M + 1)) if tails and (M + 1) * n_max * max(1, D) <= (1 << 24) else None
    if tails and tl is None:
        tl = np.empty(1)      # (refused by the library before it is written: more than 2^24 doubles)
    L = selftest_lib()
    if L.amwg_loo_check(device, _dp(dr), rows, PR, Cn, D, mds, scratch_bytes, _dp(summary), high.ctypes.data_as(C.POINTER(C.c_int32)),
                        _dp(pw) if pointwise else None, _dp(tl) if tails else None) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    out = {"summary": summary, "high": high}
    if pointwise:
        out["pointwise"] = pw
    if tails:
        out["tails"] = tl
    return out


def loo_stats(timing=False):
    """libamwg_selftest.so: (select passes over the terms, [ms of the lppd pass, the select, the compaction, the sort and fit] or None unless timing was on) of this
    process's last LOO call; then switches the phase timing of later calls on or off (amwg_loo_stats)"""
    passes, ms = C.c_int32(0), np.zeros(4)
    selftest_lib().amwg_loo_stats(1 if timing else 0, C.byref(passes), _dp(ms))
    return int(passes.value), (None if ms[0] < 0 else ms.tolist())


def hpd_limits(scratch_bytes=0, device=0, lds=True):
    """libamwg_selftest.so: sets the scratch budget of later hpd_check calls (0: the default) -> (keys one workgroup sorts in LDS on `device`, or None with
    lds=False, which opens no device; the budget in force before) (amwg_hpd_limits)"""
    L = selftest_lib()
    keys, before = C.c_int64(0), C.c_int64(0)
    if L.amwg_hpd_limits(device, scratch_bytes, C.byref(keys) if lds else None, C.byref(before)) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return (keys.value if lds else None), before.value


def fold_check(draws, D, window_rows, device=0):
    """libamwg_selftest.so: the fold of Sampler.summarize on any array draws [rows][PR][C], in windows of window_rows, beside chain_halves_kernel on the whole
    array -> halves_folded, halves_direct (arrays [2 halves][mean | variance][PR][C]), mean, sd ([D][PR], D datasets of C / D columns each) (amwg_fold_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    rows, PR, Cn = dr.shape
    hf, hd = np.empty((2, 2, PR, Cn)), np.empty((2, 2, PR, Cn))
    m, sd = np.empty((D, PR)), np.empty((D, PR))
    L = selftest_lib()
    if L.amwg_fold_check(device, _dp(dr), rows, PR, Cn, D, window_rows, _dp(hf), _dp(hd), _dp(m), _dp(sd)) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return hf, hd, m, sd


def summaries_check(draws, D, window_rows=0, device=0):
    """libamwg_selftest.so: the stored-draw summaries on any array draws [rows][PR][C], D datasets of C / D columns each, through the launchers behind
    Sampler.dataset_moments / dataset_convergence / convergence; window_rows > 0: the halves from the fold of Sampler.summarize instead of chain_halves_kernel
    -> dict of mean, sd, rhat_ds, ess_ds ([D][PR]) and rhat_pooled, ess_pooled ([PR], over all C columns) (amwg_summaries_check)"""
    dr = np.ascontiguousarray(draws, dtype=np.float64)
    rows, PR, Cn = dr.shape
    out = {k: np.empty((D, PR)) for k in ("mean", "sd", "rhat_ds", "ess_ds")}
    out.update({k: np.empty(PR) for k in ("rhat_pooled", "ess_pooled")})
    L = selftest_lib()
    if L.amwg_summaries_check(device, _dp(dr), rows, PR, Cn, D, window_rows, *[_dp(out[k]) for k in ("mean", "sd", "rhat_ds", "ess_ds", "rhat_pooled", "ess_pooled")]) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return out


def _group(samplers):
    arr = (C.c_void_p * len(samplers))(*[s.h for s in samplers])
    return arr, len(samplers), samplers[0].PR


def group_moments(samplers):
    """mean, sd over the pooled draws of several samplers (the shards of one job): amwg_group_moments (RCCL all-reduce)"""
    arr, n, PR = _group(samplers)
    m, sd = np.empty(PR), np.empty(PR)
    _check(lib().amwg_group_moments(arr, n, _dp(m), _dp(sd)))
    return m, sd


def group_convergence(samplers):
    arr, n, PR = _group(samplers)
    r, e = np.empty(PR), np.empty(PR)
    _check(lib().amwg_group_diagnostics(arr, n, _dp(r), _dp(e)))
    return r, e


def group_quantiles(samplers, probs):
    arr, n, PR = _group(samplers)
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    out = np.empty((PR, pr.size))
    _check(lib().amwg_group_quantiles(arr, n, _dp(pr), pr.size, _dp(out)))
    return out


def group_gather_draws(samplers, root=0, dst_device=None, to_host=True):
    """amwg_group_gather_draws: the recorded draws of every shard on the device of shard `root`, blocks back to back in shard order
    -> (list of per-shard arrays [kept][P + derived][chains_i] if to_host else None, offsets)"""
    arr, n, PR = _group(samplers)
    rows = samplers[0]._pending
    sizes = [rows * PR * s.C for s in samplers]
    total = sum(sizes)
    host = np.empty(total, dtype=np.float64) if to_host else None
    offs = (C.c_int64 * n)()
    _check(lib().amwg_group_gather_draws(arr, n, root, C.c_void_p(dst_device) if dst_device else None, _dp(host) if to_host else None, total * 8, offs))
    blocks = None
    if to_host:
        blocks = [host[offs[i]:offs[i] + sizes[i]].reshape(rows, PR, samplers[i].C) for i in range(n)]
    return blocks, list(offs)


def group_comm_info(samplers):
    arr, n, _ = _group(samplers)
    nr = C.c_int32()
    devs = (C.c_int32 * max(n, 1))()
    _check(lib().amwg_group_comm_info(arr, n, C.byref(nr), devs, n))
    return {"rccl_ranks_seen": nr.value, "devices": [devs[i] for i in range(min(n, nr.value))]}


class Comm:
    """A communicator over the processes of a one-process-per-device job (amwg_comm_*).  `exchange(id_bytes_or_None) -> id_bytes` carries rank 0's
    128-byte id to every rank (e.g. a torch.distributed broadcast)."""

    def __init__(self, n_ranks, rank, device, exchange):
        buf = C.create_string_buffer(128)
        if rank == 0:
            _check(lib().amwg_comm_unique_id(buf, 128))
        ident = exchange(buf.raw if rank == 0 else None)
        h = C.c_void_p()
        _check(lib().amwg_comm_create(ident, len(ident), n_ranks, rank, device, C.byref(h)))
        self.h, self.n_ranks, self.rank = h, n_ranks, rank

    def info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().amwg_comm_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"rccl_ranks_seen": a.value, "rank": b.value, "device": c.value}

    def gather_draws(self, sampler, root, dst_device_ptr, capacity_bytes):
        counts = (C.c_int64 * self.n_ranks)()
        _check(lib().amwg_comm_gather_draws(sampler.h, self.h, root, C.c_void_p(dst_device_ptr) if dst_device_ptr else None, capacity_bytes, counts))
        return list(counts)

    def moments(self, sampler):
        m, s = np.empty(sampler.PR), np.empty(sampler.PR)
        _check(lib().amwg_comm_moments(sampler.h, self.h, _dp(m), _dp(s)))
        return m, s

    def close(self):
        if getattr(self, "h", None):
            lib().amwg_comm_destroy(self.h)
            self.h = None


def code_cache_stats():
    """(hits, misses, directory) of the on-disk cache of compiled closures in this process."""
    h, m = C.c_int64(0), C.c_int64(0)
    buf = C.create_string_buffer(1024)
    _check(lib().amwg_code_cache_stats(C.byref(h), C.byref(m), buf, 1024))
    return h.value, m.value, buf.value.decode()


def fp64_peak(device=0):
    """Measured fp64 fma issue rate of the device, lane-operations per second."""
    v = C.c_double()
    _check(lib().amwg_fp64_peak(device, C.byref(v)))
    return v.value


STREAM_CHAIN, STREAM_PAIRS, STREAM_WINDOW, STREAM_WINDOW_AT = 0, 100, 200, 201      # amwg_stream_check's kinds beside CoopStream<G>::next, whose kind is G


def stream_check(kind, seed, chain0, consumed0, n_draws, calls=None, device=0):
    """libamwg_selftest.so: the product's uniform-stream classes on the device, chain i with id chain0 + i from position consumed0[i] (amwg_stream_check).
    kind: STREAM_CHAIN, a lane count G of CoopStream<G> (1 .. 64), STREAM_PAIRS (CoopStream<1> under calls: 0 = next(), 1 = next_pair()), STREAM_WINDOW,
    STREAM_WINDOW_AT -> dict of draws [chains][n_draws], consumed [chains]; for STREAM_WINDOW_AT also ahead [chains][128] (at() after ensure_b()), window
    [chains][256] (at() after a shift() and the next ensure_b()) and flags [chains][3][4]: EA, OA, EB, OB after ensure_b(), shift(), ensure_b()."""
    c0 = np.ascontiguousarray(consumed0, dtype=np.uint64)
    n = c0.size
    width = n_draws + (384 if kind == STREAM_WINDOW_AT else 0)
    out = np.empty((n, width))
    cons = np.empty(n, dtype=np.uint64)
    flags = np.empty((n, 3, 4), dtype=np.uint64) if kind == STREAM_WINDOW_AT else None
    cl = np.ascontiguousarray(calls, dtype=np.uint8) if calls is not None else None
    pu64 = C.POINTER(C.c_uint64)
    L = selftest_lib()
    if L.amwg_stream_check(device, kind, seed, chain0, n, c0.ctypes.data_as(pu64), n_draws, cl.ctypes.data_as(C.POINTER(C.c_uint8)) if cl is not None else None,
                           cl.size if cl is not None else 0, _dp(out), cons.ctypes.data_as(pu64), flags.ctypes.data_as(pu64) if flags is not None else None) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    res = {"draws": out[:, :n_draws], "consumed": cons}
    if flags is not None:
        res.update(ahead=out[:, n_draws:n_draws + 128], window=out[:, n_draws + 128:], flags=flags)
    return res


def two_valued_sum_check(x, acc0, l1, l0, device=0):
    """libamwg_selftest.so: csrc/amwg_twoval.h two_valued_sum and the plain loop acc = acc + (x[i] ? l1 : l0), both on the device, lane j from acc0[j] with the
    addends l1[j], l0[j] over the observations x [n] (0 / 1), on the library's own tables -> (fast_forward [m], term_by_term [m])  (amwg_two_valued_sum_check)"""
    xs = np.ascontiguousarray(x, dtype=np.float64)
    a0, a1, b0 = (np.ascontiguousarray(v, dtype=np.float64) for v in (acc0, l1, l0))
    if xs.ndim != 1 or a0.ndim != 1 or a1.shape != a0.shape or b0.shape != a0.shape:
        raise AmwgError("amwg error: two_valued_sum_check: x [n], acc0, l1 and l0 [m]")
    ff, seq = np.empty(a0.size), np.empty(a0.size)
    L = selftest_lib()
    if L.amwg_two_valued_sum_check(device, _dp(xs), xs.size, a0.size, _dp(a0), _dp(a1), _dp(b0), _dp(ff), _dp(seq)) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return ff, seq


def two_valued_tables(x):
    """libamwg_selftest.so: the library's own two_valued_tables (csrc/amwg_create.hip) for the observations x [n] (bytes, non-zero = 1) -> uint32 [6 (n // 32 + 2)]:
    w, pre, om1, po1, om0, po0 back to back.  Host only  (amwg_two_valued_tables)"""
    xb = np.ascontiguousarray(x, dtype=np.uint8)
    if xb.ndim != 1:
        raise AmwgError("amwg error: two_valued_tables: x [n]")
    out = np.empty(6 * (xb.size // 32 + 2), dtype=np.uint32)
    L = selftest_lib()
    if L.amwg_two_valued_tables(xb.ctypes.data_as(C.POINTER(C.c_uint8)), xb.size, out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return out


def k_valued_sum_check(K, idx, tab, acc0, c, device=0):
    """libamwg_selftest.so: csrc/amwg_kval.h k_valued_sum<K> and the plain loop acc = acc + c[idx[i]], both on the device, lane j from acc0[j] with the addends
    c[j][0 .. K - 1] over the value indices idx[n] (uint8) and the caller's own table words tab (uint32, 2 K (n // 32 + 2)) -> (fast_forward [m], term_by_term [m])
    (amwg_k_valued_sum_check)"""
    ix = np.ascontiguousarray(idx, dtype=np.uint8)
    tb = np.ascontiguousarray(tab, dtype=np.uint32)
    a0 = np.ascontiguousarray(acc0, dtype=np.float64)
    cc = np.ascontiguousarray(c, dtype=np.float64)
    if ix.ndim != 1 or a0.ndim != 1 or cc.shape != (a0.size, K) or tb.size != 2 * K * (ix.size // 32 + 2):
        raise AmwgError("amwg error: k_valued_sum_check: idx [n], acc0 [m], c [m][K] and tab of 2 K (n // 32 + 2) words")
    ff, seq = np.empty(a0.size), np.empty(a0.size)
    L = selftest_lib()
    if L.amwg_k_valued_sum_check(device, K, ix.ctypes.data_as(C.POINTER(C.c_uint8)), ix.size, tb.ctypes.data_as(C.POINTER(C.c_uint32)), a0.size, _dp(a0), _dp(cc), _dp(ff), _dp(seq)) != 0:
        raise AmwgError("amwg error: %s" % L.amwg_last_error().decode())
    return ff, seq


def device_eval(op, a, b=None, c=None, device=0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bb = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
    cc = np.ascontiguousarray(c, dtype=np.float64) if c is not None else None
    _check(selftest_lib().amwg_device_eval(device, op, a.size, _dp(a), _dp(bb) if bb is not None else None,
                                  _dp(cc) if cc is not None else None, _dp(out)))
    return out
