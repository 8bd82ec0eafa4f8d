'use strict';
// dataset_predictive(), predictive() and pit_histogram() on the GPU: three training folds of the README Normal closure in ONE ragged sampler, every fold scored on what
// it has not seen and on its own data.  The four pointwise values against the rule of include/amwg.h restated over sample()'s array; the summary against the finish.
// THE TOLERANCES are the header's plus this restatement's own error: it sums S doubles (another E = 8 (S + 16) u on the means), and its erfc is Abramowitz & Stegun
// 7.1.26, whose published error is 1.5e-7 -- the distribution function itself is held to 2^-49 by tests/test_gpu_predictive.py; here the front end is.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;

var params = { mu: {type: "real"}, sigma: {type: "real", lower: 0} };
var log_post = function(state, data) {      // the README closure, in the form the front end recognises as the Normal family
  var log_post = 0;
  log_post += ld.norm(state.mu, 0, 100);
  log_post += ld.unif(state.sigma, 0, 100);
  for(var i = 0; i < data.length; i++) {
    log_post += ld.norm(data[i], state.mu, state.sigma);
  }
  return log_post;
};

const N = mcmc.native(), K = 3, CPD = 64, KEPT = 14, U = Math.pow(2, -53), message = (e) => String(e && e.message ? e.message : e);
const x = [];
for (let i = 0; i < 40; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(952, 1, i * 12 + k); x.push(170 + 7 * (s - 6)); }
const test = [x.slice(0, 13), x.slice(13, 14), x.slice(14)], train = test.map((_, k) => x.filter((_, i) => !(k === 0 ? i < 13 : k === 1 ? i === 13 : i >= 14)));
const common = { seed: 20261127, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(200); s.thin(3); return s.sample(40); }
function cdf(z) {      // 0.5 erfc(-z / sqrt 2)
  const v = Math.abs(z) * Math.SQRT1_2, t = 1 / (1 + 0.3275911 * v);
  const tail = 0.5 * t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429)))) * Math.exp(-v * v);
  return z < 0 ? tail : 1 - tail;
}
function check(entry, xs, mu, sigma) {
  const S = mu.length, E = 8 * (S + 16) * U, mean = (f) => { let a = 0; for (let s = 0; s < S; s++) a += f(s); return a / S; };
  assert.deepStrictEqual(Object.keys(entry), ['cover50', 'cover90', 'rmse', 'mean_mid', 'n', 'pointwise']);
  const n = xs.length, pm = mean((s) => mu[s]), top = Math.max(...Array.from(sigma, (q, s) => q * q + mu[s] * mu[s]));
  const var_ = mean((s) => sigma[s] * sigma[s]) + mean((s) => (mu[s] - pm) * (mu[s] - pm));
  let in50 = 0, in90 = 0, ss = 0, mids = 0;
  xs.forEach((xj, j) => {
    const p = entry.pointwise[j], pit = mean((s) => cdf((xj - mu[s]) / sigma[s]));
    assert.ok(Object.is(p.pit_hi, p.pit_lo) && Math.abs(p.pit_hi - pit) <= E + Math.pow(2, -49) + 1.5e-7, 'observation ' + j + ': ' + p.pit_hi + ' vs ' + pit);
    assert.ok(Math.abs(p.pred_mean - pm) <= 2 * E * Math.abs(pm) && Math.abs(p.pred_sd * p.pred_sd - var_) <= 8 * E * top, JSON.stringify(p) + ' vs ' + pm + ' ' + var_);
    const mid = (p.pit_hi + p.pit_lo) / 2;
    in50 += 0.25 <= mid && mid <= 0.75 ? 1 : 0; in90 += 0.05 <= mid && mid <= 0.95 ? 1 : 0; ss += (xj - p.pred_mean) * (xj - p.pred_mean); mids += mid;
  });
  assert.ok(entry.n === n && entry.pointwise.length === n && Object.is(entry.cover50, in50 / n) && Object.is(entry.cover90, in90 / n) && Object.is(entry.rmse, Math.sqrt(ss / n)) && Object.is(entry.mean_mid, mids / n), JSON.stringify(entry));
}

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets: train, chains: K * CPD }, common));
const got = run(all);
const folds = all.dataset_predictive({ data: test }), own = all.dataset_predictive();
for (let d = 0; d < K; d++) {
  const mu = new Float64Array(KEPT * CPD), sigma = new Float64Array(KEPT * CPD);      // this dataset's slice of sample()'s [kept][chains], draw s = row * CPD + chain
  for (let t = 0; t < KEPT; t++) {
    mu.set(got.mu.subarray(t * K * CPD + d * CPD, t * K * CPD + (d + 1) * CPD), t * CPD);
    sigma.set(got.sigma.subarray(t * K * CPD + d * CPD, t * K * CPD + (d + 1) * CPD), t * CPD);
  }
  check(folds[d], test[d], mu, sigma);
  check(own[d], train[d], mu, sigma);
}
assert.ok(!('pointwise' in all.dataset_predictive({ data: test, pointwise: false })[0]));
// the histogram: continuous PITs fall into one bin each; a count's step is spread over the bins it covers; 1 falls into the last bin; NaN is left out
const hist = mcmc.pit_histogram([].concat(...folds.map((f) => f.pointwise)), 5);      // (continuous PITs: whole counts that add up to the observations)
assert.ok(hist.length === 5 && hist.reduce((a, b) => a + b, 0) === x.length && hist.every((h) => h === Math.floor(h)));
assert.deepStrictEqual(mcmc.pit_histogram([{ pit_lo: 0.125, pit_hi: 0.375 }, { pit_lo: 1, pit_hi: 1 }, { pit_lo: NaN, pit_hi: NaN }, { pit_lo: 0, pit_hi: 1 }], 4), [0.75, 0.75, 0.25, 1.25]);
assert.throws(() => mcmc.pit_histogram(null, 4), /pit_histogram/);
assert.throws(() => all.predictive(), (e) => /datasets/.test(message(e)));
all.close();
// an ordinary sampler: predictive() is the one entry of dataset_predictive()
const one = new mcmc.AmwgSampler(params, log_post, train[0], Object.assign({ chains: CPD }, common));
const kept = run(one);
check(one.predictive({ data: test[0] }), test[0], kept.mu, kept.sigma);
one.close();
// a translated closure is refused by the front end and by the library, in the same words
const closure = new mcmc.AmwgSampler(params, log_post, train[0], Object.assign({ chains: CPD, translate: true }, common));
const refused = (e) => /dataset_predictive/.test(message(e)) && /predictive distribution of a closure is not known to the library; built-in families only/.test(message(e));
assert.throws(() => closure.dataset_predictive(), refused);
assert.throws(() => N.datasetPredictive(closure._shards[0].handle, null, null, false), refused);
closure.close();
