'use strict';
// dataset_hpd() and hpd() of the JavaScript front end on the GPU: the README Normal closure on three datasets x 64 chains in ONE sampler (options.datasets).
// One entry per dataset, shaped like dataset_quantiles() with a pair [lo, hi] per probability, deep-equal (Object.is on every number) to the rule of
// include/amwg.h restated here over that dataset's slice of the array sample() returned: the same doubles.  The pooled hpd() throws on the dataset sampler;
// after summarize() both throw the library's refusal.  On an ordinary sampler with a derived quantity hpd() is the one entry of dataset_hpd(), name by name.
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

const N = mcmc.native(), D = 3, CPD = 64, SEED = 20261020, NOBS = 300, KEPT = 14, PROBS = [0.5, 0.95];
const datasets = [];
for (let d = 0; d < D; d++) {      // seeded synthetic heights: sums of twelve Philox uniforms around a mean that differs per dataset
  const x = [];
  for (let i = 0; i < NOBS; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(900 + d, 1, i * 12 + k); x.push(170 + 5 * d + 7 * (s - 6)); }
  datasets.push(x);
}
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(120); s.thin(3); return s.sample(40); }

// the rule: g = floor(p n) clamped to [1, n - 1]; the first smallest of w_i = x_(i+g) - x_(i), i < n - g.  (A Float64Array sorts -0 before +0.)
function hpd(sorted, p) {
  const n = sorted.length;
  if (!(p > 0 && p < 1)) return [NaN, NaN];
  for (let i = 0; i < n; i++) if (!Number.isFinite(sorted[i])) return [NaN, NaN];
  const g = Math.min(Math.max(Math.floor(p * n), 1), n - 1);
  let best = 0;
  for (let i = 1; i < n - g; i++) if (sorted[i + g] - sorted[i] < sorted[best + g] - sorted[best]) best = i;
  return [sorted[best], sorted[best + g]];
}
const message = (e) => String(e && e.message ? e.message : e);

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets, chains: D * CPD }, common));
const got = run(all);
assert.strictEqual(got.mu.layout.kept, KEPT);
const dh = all.dataset_hpd(PROBS), dq = all.dataset_quantiles(PROBS);
assert.strictEqual(dh.length, D);
for (let d = 0; d < D; d++) {
  assert.deepStrictEqual(Object.keys(dh[d]), Object.keys(dq[d]));
  const want = {};
  for (const name of Object.keys(dq[d])) {
    assert.strictEqual(dh[d][name].length, dq[d][name].length);      // elements
    const seg = new Float64Array(KEPT * CPD);      // this dataset's slice of sample()'s [kept][chains]
    for (let t = 0; t < KEPT; t++) seg.set(got[name].subarray(t * D * CPD + d * CPD, t * D * CPD + (d + 1) * CPD), t * CPD);
    seg.sort();
    want[name] = [PROBS.map((p) => hpd(seg, p))];
    dh[d][name][0].forEach((pair, k) => assert.ok(pair.length === 2 && pair[0] <= pair[1], name + ' p ' + PROBS[k]));
    assert.ok(dh[d][name][0][1][1] - dh[d][name][0][1][0] >= dh[d][name][0][0][1] - dh[d][name][0][0][0]);      // the 95 % interval is no narrower than the 50 % one
  }
  assert.deepStrictEqual(dh[d], want);
}
assert.throws(() => all.hpd(PROBS), (e) => /datasets/.test(message(e)));
all.summarize(40);
const refusal = (e) => /amwg_last_sample_dataset_hpd/.test(message(e)) && /amwg_sample_summarize/.test(message(e));
assert.throws(() => all.dataset_hpd(PROBS), refusal);
all.close();

// an ordinary sampler of a translated closure with a derived quantity (`var`, recorded after the parameters)
const um = require('./user_models.js');
const m = um.build('norm_post_derived');
const der = new mcmc.AmwgSampler(m.params, m.log_post, m.data, { seed: 5, chains: 64, lanes_per_chain: 4, translate: true });
der.burn(200);
const draws = der.sample(60);
const one = der.dataset_hpd(PROBS), pooled = der.hpd(PROBS), shape = der.quantiles(PROBS);
assert.strictEqual(one.length, 1);
assert.deepStrictEqual(one[0], pooled);
assert.deepStrictEqual(Object.keys(pooled), Object.keys(shape));
assert.ok(Object.keys(pooled).indexOf('var') >= 0);
for (const name of Object.keys(pooled)) {
  assert.strictEqual(pooled[name].length, shape[name].length);
  pooled[name].forEach((row, e) => { assert.strictEqual(row.length, PROBS.length); row.forEach((pair) => assert.strictEqual(pair.length, 2)); });
}
const v = Float64Array.from(draws['var']).sort();
assert.deepStrictEqual(pooled['var'], [PROBS.map((p) => hpd(v, p))]);
der.summarize(20);
assert.throws(() => der.hpd(PROBS), refusal);
der.close();
console.log('gpu hpd ok');
