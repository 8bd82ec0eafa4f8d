// (sloppy mode on purpose, like user_models.js: the closures are written against a global `ld`)
/*
 * dataset_models.js -- TEST FIXTURES: closures on D = 3 datasets of equal shape, for options.datasets with a translated closure (translate.js translate_datasets,
 * amwg_create_user_datasets).  build(name) -> {params, datasets, log_post}; the data comes from fixed seeds.  Used by tests/js/translate_datasets_cli.js (which writes
 * source, meta and per-dataset arrays for the Python tests) and by tests/js/test_gpu_user_datasets.js.
 */
const synth = require('../../oracle/synth.js');

function lcg(seed) { let s = seed >>> 0; return () => { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; }; }
const D = 3;
const CASES = {};

// the closure no family recognises of tests/test_datasets_host.py (`ld.norm(x[i] * 2, mu, sigma)`), N = 37
CASES.ds_scaled_normal = {
  params: () => ({ mu: { type: 'real' }, sigma: { type: 'real', lower: 0 } }),
  datasets: (n, count) => Array.from({ length: count || D }, (_, d) => Array.from(synth.normal(n || 37, 20261019 + d).x)),      // (tools/time_user_datasets.py: other sizes and counts)
  log_post: function (state, data) { var lp = ld.norm(state.mu, 0, 100) + ld.unif(state.sigma, 0, 100); for (var i = 0; i < data.length; i++) lp += ld.norm(data[i] * 2, state.mu, state.sigma); return lp; },
};

// the README's Normal closure, forced through the translator: it ends in the constant-mean normal loop, so it must come out with a certified tail
CASES.ds_readme_normal = {
  params: () => ({ mu: { type: 'real' }, sigma: { type: 'real', lower: 0 } }),
  datasets: () => Array.from({ length: D }, (_, d) => Array.from(synth.normal(37, 20261119 + d).x)),
  log_post: function(state, data) {
    var log_post = 0;
    // Priors
    log_post += ld.norm(state.mu, 0, 100);
    log_post += ld.unif(state.sigma, 0, 100);
    // Likelihood
    for(var i = 0; i < data.length; i++) {
      log_post += ld.norm(data[i], state.mu, state.sigma);
    }
    return log_post;
  },
};

// counts y (N = 70 = 64 + 6: crosses a wavefront's share), a double covariate, labels g into theta[3], a scalar that differs between the datasets (offset), one that
// does not (scale), one derived quantity.  Dataset 0: y <= 255, labels {0, 1}; dataset 1: one y = 300, labels {0, 1, 2}; dataset 2: one y = 2.5 (ld.pois takes it as it
// comes: a finite term through lgamma) and one y = -1 (the term is -Infinity, as in JavaScript: log_post is -Infinity at every state and the chains of that dataset
// never move).  So the storage types of y are u8 / i32 / f64 and the ranges of g differ: the union matters.
CASES.ds_mixed = {
  params: () => ({ theta: { type: 'real', dim: [3], init: 0.1 }, b: { type: 'real', init: 0.1 } }),
  datasets: () => Array.from({ length: D }, (_, d) => {
    const r = lcg(777 + d), N = 70, y = [], x = [], g = [];
    for (let i = 0; i < N; i++) { y.push(Math.floor(r() * 6)); x.push(r() * 2 - 1); g.push(Math.floor(r() * (d === 0 ? 2 : 3))); }
    if (d === 1) { y[5] = 300; g[0] = 2; }
    if (d === 2) { y[7] = 2.5; y[9] = -1; g[1] = 2; }
    return { y, x, g, offset: 0.125 * d - 0.25, scale: 0.5 };
  }),
  log_post: function (state, data) {
    var lp = ld.norm(state.b, 0, 10);
    for (var k = 0; k < 3; k++) lp += ld.norm(state.theta[k], 0, 10);
    for (var i = 0; i < data.y.length; i++) {
      lp += ld.pois(data.y[i], Math.exp(state.theta[data.g[i]] + state.b * data.x[i] * data.scale + data.offset));
    }
    state.spread = state.theta[2] - state.theta[0];
    return lp;
  },
};

// 18 arrays of length 5: two more than the pointers that travel in the kernel arguments
const MANY = 18;
CASES.ds_many_arrays = {
  params: () => ({ mu: { type: 'real' }, sigma: { type: 'real', lower: 0, init: 1 } }),
  datasets: () => Array.from({ length: D }, (_, d) => { const r = lcg(4242 + d), o = {}; for (let j = 0; j < MANY; j++) o['a' + j] = Array.from({ length: 5 }, () => r() * 4 - 2 + j * 0.25); return o; }),
  log_post: eval('(function (state, data) { var lp = ld.norm(state.mu, 0, 100) + ld.unif(state.sigma, 0, 100); for (var i = 0; i < 5; i++) lp += ld.norm(' +
                 Array.from({ length: MANY }, (_, j) => 'data.a' + j + '[i]').join(' + ') + ', state.mu, state.sigma); return lp; })'),
};

// ---- what translate_datasets refuses
// unequal shapes
CASES.bad_shapes = {
  params: CASES.ds_scaled_normal.params,
  datasets: () => [[1, 2, 3, 4], [2, 3, 4, 5, 6], [1, 2, 3, 4]],
  log_post: CASES.ds_scaled_normal.log_post,
};
// a loop bound taken from a scalar that differs
CASES.bad_loop_bound = {
  params: CASES.ds_scaled_normal.params,
  datasets: () => [{ n: 3, x: [1, 2, 3, 4] }, { n: 4, x: [2, 3, 4, 5] }, { n: 3, x: [1, 2, 3, 4] }],
  log_post: function (state, data) { var lp = ld.norm(state.mu, 0, 100) + ld.unif(state.sigma, 0, 100); for (var i = 0; i < data.n; i++) lp += ld.norm(data.x[i], state.mu, state.sigma); return lp; },
};
// string levels that differ
CASES.bad_levels = {
  params: CASES.ds_scaled_normal.params,
  datasets: () => [{ arm: ['a', 'b', 'a', 'b'], x: [1, 2, 3, 4] }, { arm: ['b', 'a', 'b', 'a'], x: [2, 3, 4, 5] }, { arm: ['a', 'b', 'a', 'b'], x: [1, 2, 3, 4] }],
  log_post: function (state, data) {
    var lp = ld.norm(state.mu, 0, 100) + ld.unif(state.sigma, 0, 100);
    for (var i = 0; i < data.x.length; i++) lp += ld.norm(data.x[i], data.arm[i] === 'a' ? state.mu : -state.mu, state.sigma);
    return lp;
  },
};

module.exports = { names: ['ds_scaled_normal', 'ds_readme_normal', 'ds_mixed', 'ds_many_arrays'], refused: ['bad_shapes', 'bad_loop_bound', 'bad_levels'],
  build: (name, n, count) => { const c = CASES[name]; if (!c) throw new Error('no such dataset model: ' + name); return { params: c.params(), datasets: c.datasets(n, count), log_post: c.log_post }; } };
