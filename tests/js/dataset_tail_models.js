// (sloppy mode on purpose, like dataset_models.js: the closures are written against a global `ld`)
/*
 * dataset_tail_models.js -- TEST FIXTURES: closures that end in a logistic-regression loop or in a log-link Poisson loop, on D = 3 datasets of equal shape, for the
 * certified tails of options.datasets with a translated closure (translate.js translate_datasets with tail_consts_array; csrc/amwg_gtail.h:
 * kTailPerDataset).  build(name[, n_obs[, n_datasets]]) -> {params, datasets, log_post}; the data comes from fixed seeds.  Used by
 * tests/js/translate_dataset_tails_cli.js, tests/js/test_gpu_user_dataset_tails.js, tools/bound_audit.py (dstail) and tools/time_user_dataset_tails.py.
 * Every slot of a dataset's constants differs between the datasets: a bound formed from dataset 0's values for everyone shows in the host test.
 */
const lm = require('./logit_models.js');

function lcg(seed) { let s = seed >>> 0; return () => { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; }; }
const D = 3;
const CASES = {};

// logit_tail_small of logit_models.js on its own data generator; 517 = 8 rounds of 64 + 5: the paired row buffers and a ragged last round
CASES.dst_logit = {
  params: lm.params,
  datasets: (n, count) => Array.from({ length: count || D }, (_, d) => lm.data(n || 517, 20261101 + d)),
  log_post: lm.CASES.logit_tail_small,
};

// real-valued weights in the place of y; dataset 2's are scaled by 2^10: sum |w| differs a thousandfold and is no integer (the rounded-up form)
CASES.dst_logit_weights = {
  params: lm.params,
  datasets: (n, count) => Array.from({ length: count || D }, (_, d) => { const o = lm.data(n || 517, 20261201 + d); if (d === 2) o.w = o.w.map((v) => v * 1024); return o; }),
  log_post: lm.CASES.logit_tail_weights,
};

// a Poisson GLM per dataset with a linear predictor (kTailLinear): counts y, three covariates (column 0 a constant that differs per dataset).  Dataset 0: counts <= 5; dataset 1: a few counts up to ~300 (the one
// source stores y as i32); dataset 2: counts <= 5, covariate column 1 all zero (its own translation prunes the term from H), column 2 scaled by 8.
function poisData(n, d, r) {
  const X = [], y = [];
  for (let i = 0; i < n; i++) {
    const x0 = 1 + 0.25 * (d % 3), x1 = r() * 2 - 1, x2 = r() * 2 - 1;
    X.push(x0, d % 3 === 2 ? 0 : x1, d % 3 === 2 ? 8 * x2 : x2);
    y.push(d % 3 === 1 && i % 16 === 3 ? 200 + Math.floor(r() * 100) : Math.floor(r() * 6));
  }
  return { X, y };
}
const poisClosure = function (s, d) {
  var lp = 0;
  for (var j = 0; j < 3; j++) lp += ld.norm(s.b[j], 0, 10);
  for (var i = 0; i < d.y.length; i++) {
    var eta = 0;
    for (var k = 0; k < 3; k++) eta += d.X[i * 3 + k] * s.b[k];
    lp += ld.pois(d.y[i], Math.exp(eta));
  }
  return lp;
};
const poisParams = () => ({ b: { dim: [3], init: 0 } });
const poisCase = (n0, seed) => ({
  params: poisParams,
  datasets: (n, count) => Array.from({ length: count || D }, (_, d) => poisData(n || n0, d, lcg(seed + d))),
  log_post: poisClosure,
});
CASES.dst_pois_linear = poisCase(65, 20261301);      // one full round + 1
CASES.dst_pois_small = poisCase(37, 20261401);       // no full round
// one negative count in dataset 2: that dataset cannot take the plan, so no dataset does
CASES.dst_pois_fallback = {
  params: poisParams,
  datasets: (n, count) => { const ds = CASES.dst_pois_linear.datasets(n, count); ds[2].y[11] = -1; return ds; },
  log_post: poisClosure,
};

// 16 data arrays (y and 15 covariates), N = 65: the constants are the 17th array, one more than the pointers that travel in the kernel arguments -- it is read
// through the device table (amwg_user.h user_arr, DataRef::arr_ext)
const COV = 15;
CASES.dst_logit_many = {
  params: lm.params,
  datasets: (n, count) => Array.from({ length: count || D }, (_, d) => {
    const r = lcg(20261501 + d), N = n || 65, o = { y: [] };
    for (let j = 0; j < COV; j++) o['a' + j] = Array.from({ length: N }, () => (r() * 2 - 1) * (j < 2 ? 1 : 0.1));
    for (let i = 0; i < N; i++) o.y.push(r() < 1 / (1 + Math.exp(-(0.2 + 0.8 * o.a0[i] - 0.5 * o.a1[i]))) ? 1 : 0);
    return o;
  }),
  log_post: eval('(function (s, d) { var lp = 0; for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10); for (var i = 0; i < d.y.length; i++) { ' +
                 'var eta = s.b[0] + s.b[1] * d.a0[i] + s.b[2] * d.a1[i] + s.b[3] * (' + Array.from({ length: COV - 2 }, (_, j) => 'd.a' + (j + 2) + '[i]').join(' + ') + '); ' +
                 'lp += d.y[i] * eta - Math.log1p(Math.exp(eta)); } return lp; })'),
};

module.exports = { names: ['dst_logit', 'dst_logit_weights', 'dst_pois_linear', 'dst_pois_small', 'dst_pois_fallback', 'dst_logit_many'], D,
  build: (name, n, count) => { const c = CASES[name]; if (!c) throw new Error('no such dataset tail model: ' + name); return { params: c.params(), datasets: c.datasets(n, count), log_post: c.log_post }; } };
