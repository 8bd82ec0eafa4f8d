"""THE RULE of amwg_last_sample_dataset_predictive (include/amwg.h) restated in plain loops with mpmath means over the draws, and the header's bounds.  What the
library fixes in IEEE doubles is formed in doubles here too: z = (x - mean) / sigma, the Poisson family's eta in the term's order of operations and
lambda = amwg_exp(eta) (the library's own exp on the host, bit for bit the device's); everything after that is exact to 30 digits."""
import mpmath as mp
import numpy as np

import amwg_ctypes
import waic_reference as wr

mp.mp.dps = 30
ERFC_REL, POIS_REL = 2.0 ** -49, 2.0 ** -29      # csrc/amwg_cdf.h: kErfcRel, kPoisRel


def poisson_pair(y, lam):
    """(P(Y <= y), P(Y <= y - 1)) by the plain sum of the masses; NaN for what is no count"""
    if not (y >= 0 and y == int(y)) or not np.isfinite(lam):
        return mp.nan, mp.nan
    masses = [mp.exp(-mp.mpf(lam)) * mp.mpf(lam) ** k / mp.factorial(k) for k in range(int(y) + 1)]
    return mp.fsum(masses), mp.fsum(masses[:-1])


def rows_of(spec, sd, positions=None):
    """(F, Fm, mean, var) of every (draw, observation) of one dataset under its draws sd [S][PR]: per observation the list over the draws"""
    model, data, m = spec["model"], spec["data"], spec["n_obs"]
    for j in range(m):
        col = []
        for w in sd:
            if model in ("normal", "hier_normal"):
                mean, sigma = (w[0], w[1]) if model == "normal" else (w[int(data["g"][j])], w[int(spec["G"]) + 1])
                with np.errstate(all="ignore"):
                    z = (np.float64(data["x"][j]) - mean) / sigma
                F = mp.erfc(-mp.mpf(float(z)) * mp.sqrt(mp.mpf(1) / 2)) / 2 if np.isfinite(z) else mp.nan
                col.append((F, F, mp.mpf(float(mean)), mp.mpf(float(sigma)) ** 2))
            elif model == "beta_bern":
                x, th = data["x"][j], mp.mpf(float(w[0]))
                col.append((1 if x == 1 else 1 - th, 1 - th if x == 1 else mp.mpf(0), th, th * (1 - th)) if x in (0, 1) else (mp.nan,) * 4)
            else:
                X = np.asarray(data["x"], dtype=np.float64).reshape(m, 7)[j]
                eta = X[0] * w[0]
                for k in range(1, 7):
                    eta = eta + X[k] * w[k]
                if (positions[j] if positions is not None else j) >= w[8]:
                    eta = eta + w[7]
                lam = amwg_ctypes.lib().amwg_exp(float(eta))
                col.append(poisson_pair(data["y"][j], lam) + (mp.mpf(lam), mp.mpf(lam)))
        yield col


def pointwise(spec, sd, positions=None):
    """-> (values [m][4] = pit_hi, pit_lo, pred_mean, pred_sd; tolerances [m][4], the last on pred_sd^2): NaN rows where a term is not finite.  Tolerances: the
    header's E = 8 (S + 16) u, plus the distribution function's bound per evaluation on the two PITs; E max |mean|; 4 E (max var + max mean^2)"""
    S, model = len(sd), spec["model"]
    E = 8.0 * (S + 16) * wr.U
    vals, tols = np.full((spec["n_obs"], 4), np.nan), np.full((spec["n_obs"], 4), np.nan)
    for j, col in enumerate(rows_of(spec, sd, positions)):
        if any(mp.isnan(v) or mp.isinf(v) for t in col for v in t):
            continue
        hi, lo, mean = (sum(t[k] for t in col) / S for k in range(3))
        var = sum(t[3] for t in col) / S + sum((t[2] - mean) ** 2 for t in col) / S
        cdf = [0.0, 0.0] if model == "beta_bern" else [ERFC_REL, ERFC_REL]
        if model == "pois_glm":
            cdf = [float(sum(POIS_REL * min(t[k], 1 - t[k]) for t in col) / S) + wr.U for k in range(2)]
        vals[j] = [float(hi), float(lo), float(mean), float(mp.sqrt(var))]
        tols[j] = [E + cdf[0], E + cdf[1], E * float(max(abs(t[2]) for t in col)), 4 * E * float(max(t[3] for t in col) + max(t[2] ** 2 for t in col))]
    return vals, tols
