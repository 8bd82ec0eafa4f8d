'use strict';
// dataset_quantiles() of the JavaScript front end on the GPU: the README Normal closure on three datasets x 64 chains in ONE sampler (options.datasets).
// One entry per dataset, each shaped like quantiles() of an ordinary sampler of the same model, its values equal to a sort of that dataset's slice of the
// array sample() returned (R's type-7 rule, the oracle of tests/test_gpu_dataset_quantiles.py); the pooled quantiles() still throws.  On an ordinary sampler with a derived
// quantity, the one entry equals the pooled quantiles() name by name.  Numbers are compared with ===, i.e. as values.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;

var params = {
  mu: {type: "real"},
  sigma: {type: "real", lower: 0} };
var log_post = function(state, data) {
  var log_post = 0;
  // Priors
  log_post += ld.norm(state.mu, 0, 100);
  log_post += ld.unif(state.sigma, 0, 100);
  // Likelihood
  for(var i = 0; i < data.length; i++) {
    log_post += ld.norm(data[i], state.mu, state.sigma);
  }
  return log_post;
};

const N = mcmc.native(), D = 3, CPD = 64, SEED = 20261018, NOBS = 300, KEPT = 14, PROBS = [0.025, 0.5, 0.975];
const datasets = [];
for (let d = 0; d < D; d++) {      // seeded synthetic heights: sums of twelve Philox uniforms around a mean that differs per dataset
  const x = [];
  for (let i = 0; i < NOBS; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(900 + d, 1, i * 12 + k); x.push(170 + 5 * d + 7 * (s - 6)); }
  datasets.push(x);
}
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(120); s.thin(3); return s.sample(40); }

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets, chains: D * CPD }, common));
const got = run(all);
assert.strictEqual(got.mu.layout.kept, KEPT);
const dq = all.dataset_quantiles(PROBS);
assert.strictEqual(dq.length, all.n_datasets);
assert.strictEqual(dq.length, D);

const one = new mcmc.AmwgSampler(params, log_post, datasets[0], Object.assign({ chains: CPD }, common));
run(one);
const shape = one.quantiles(PROBS);
one.close();

function type7(sorted, q) {
  const n = sorted.length, h = (n - 1) * q, lo = Math.floor(h), hi = Math.min(lo + 1, n - 1);
  return sorted[lo] + (h - lo) * (sorted[hi] - sorted[lo]);
}
for (let d = 0; d < D; d++) {
  assert.deepStrictEqual(Object.keys(dq[d]), Object.keys(shape));
  for (const name of Object.keys(shape)) {
    assert.strictEqual(dq[d][name].length, shape[name].length);
    dq[d][name].forEach((row, e) => assert.strictEqual(row.length, shape[name][e].length));
    const seg = new Float64Array(KEPT * CPD);      // this dataset's slice of sample()'s [kept][chains]
    for (let t = 0; t < KEPT; t++) seg.set(got[name].subarray(t * D * CPD + d * CPD, t * D * CPD + (d + 1) * CPD), t * CPD);
    seg.sort();
    PROBS.forEach((q, k) => assert.ok(dq[d][name][0][k] === type7(seg, q), 'dataset ' + d + ' ' + name + ' q ' + q));      // (=== on numbers: -0 equals +0)
  }
}
assert.throws(() => all.quantiles(PROBS), (e) => /amwg_last_sample_dataset_quantiles/.test(String(e && e.message ? e.message : e)));
all.close();

// an ordinary sampler of a translated closure with a derived quantity (`var`, recorded after the parameters): one entry, the pooled quantiles() of every name
const um = require('./user_models.js');
const m = um.build('norm_post_derived');
const der = new mcmc.AmwgSampler(m.params, m.log_post, m.data, { seed: 5, chains: 64, lanes_per_chain: 4, translate: true });
der.burn(200);
der.sample(60);
const dd = der.dataset_quantiles(PROBS), pooled = der.quantiles(PROBS);
assert.strictEqual(dd.length, 1);
assert.deepStrictEqual(Object.keys(dd[0]), Object.keys(pooled));
assert.ok(Object.keys(pooled).indexOf('var') >= 0);
for (const name of Object.keys(pooled)) {
  assert.strictEqual(dd[0][name].length, pooled[name].length);
  pooled[name].forEach((row, e) => { assert.strictEqual(dd[0][name][e].length, row.length); row.forEach((v, k) => assert.ok(dd[0][name][e][k] === v, name + ' q ' + PROBS[k])); });
}
der.close();
console.log('gpu dataset quantiles ok');
