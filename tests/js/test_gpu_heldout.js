'use strict';
// dataset_heldout(), heldout() and kfold_total() on the GPU: three training folds of the README Normal closure in ONE ragged sampler, every fold scored on what it has
// not seen.  lppd_j against the rule of include/amwg.h restated over sample()'s array within the header's bound; the totals and kfold_total against the finish rule.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;

var params = {
  mu: {type: "real"},
  sigma: {type: "real", lower: 0} };
var log_post = function(state, data) {
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
for (let i = 0; i < 40; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(951, 1, i * 12 + k); x.push(170 + 7 * (s - 6)); }
const test = [x.slice(0, 13), x.slice(13, 14), x.slice(14)], train = test.map((_, k) => x.filter((_, i) => !(k === 0 ? i < 13 : k === 1 ? i === 13 : i >= 14)));
const common = { seed: 20261126, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(200); s.thin(3); return s.sample(40); }
function finish(v) {
  const n = v.length;
  let elpd = 0, ss = 0;
  for (let j = 0; j < n; j++) elpd += v[j];
  for (let j = 0; j < n; j++) ss += (v[j] - elpd / n) * (v[j] - elpd / n);
  return [elpd, n < 2 ? NaN : Math.sqrt(n * ss / (n - 1))];
}
function check(entry, xs, mu, sigma) {
  const S = mu.length, E = 8 * (S + 16) * U;
  assert.deepStrictEqual(Object.keys(entry), ['elpd_heldout', 'se', 'n', 'pointwise']);
  assert.strictEqual(entry.n, xs.length);
  assert.strictEqual(entry.pointwise.length, xs.length);
  xs.forEach((xj, j) => {
    const l = Array.from(mu, (m, s) => ld.norm(xj, m, sigma[s])), top = Math.max(...l);
    let sum = 0, c = 0;
    for (const v of l) { const e = Math.exp(v - top), t = sum + e; c += (sum - t) + e; sum = t; }
    const lppd = top + Math.log(sum + c) - Math.log(S);
    assert.ok(Math.abs(entry.pointwise[j] - lppd) <= E + 4 * U * Math.abs(lppd), 'observation ' + j + ': ' + entry.pointwise[j] + ' vs ' + lppd);
  });
  const [elpd, se] = finish(entry.pointwise);
  assert.ok(Object.is(entry.elpd_heldout, elpd) && Object.is(entry.se, se), entry.elpd_heldout + ' ' + entry.se + ' vs ' + elpd + ' ' + se);
}

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets: train, chains: K * CPD }, common));
const got = run(all);
const folds = all.dataset_heldout(test, { pointwise: true }), plain = all.dataset_heldout(test);
for (let d = 0; d < K; d++) {
  const mu = new Float64Array(KEPT * CPD), sigma = new Float64Array(KEPT * CPD);      // this dataset's slice of sample()'s [kept][chains], draw s = row * CPD + chain
  for (let t = 0; t < KEPT; t++) {
    mu.set(got.mu.subarray(t * K * CPD + d * CPD, t * K * CPD + (d + 1) * CPD), t * CPD);
    sigma.set(got.sigma.subarray(t * K * CPD + d * CPD, t * K * CPD + (d + 1) * CPD), t * CPD);
  }
  check(folds[d], test[d], mu, sigma);
  assert.ok(!('pointwise' in plain[d]) && Object.is(plain[d].elpd_heldout, folds[d].elpd_heldout) && Object.is(plain[d].se, folds[d].se));
}
assert.ok(folds.length === K && Number.isNaN(folds[1].se));      // one held-out observation has no standard error
const total = mcmc.kfold_total(folds), [elpd, se] = finish([].concat(...folds.map((f) => f.pointwise)));
assert.ok(Object.is(total.elpd_kfold, elpd) && Object.is(total.se, se) && total.n === x.length);
assert.throws(() => all.heldout(test[0]), (e) => /datasets/.test(message(e)));
all.close();
// an ordinary sampler: heldout() is the one entry of dataset_heldout()
const one = new mcmc.AmwgSampler(params, log_post, train[0], Object.assign({ chains: CPD }, common));
const kept = run(one);
check(one.heldout(test[0], { pointwise: true }), test[0], kept.mu, kept.sigma);
one.close();
// a translated closure is refused by the front end and by the library, in the same words
const closure = new mcmc.AmwgSampler(params, log_post, train[0], Object.assign({ chains: CPD, translate: true }, common));
const refused = (e) => /dataset_heldout/.test(message(e)) && /built-in families only/.test(message(e));
assert.throws(() => closure.dataset_heldout(test[0]), refused);
assert.throws(() => N.datasetHeldout(closure._shards[0].handle, [{ model: 1, n_obs: 1, G: 0, K: 0, x: Float64Array.of(170), hyper: new Float64Array(8) }], null, false), refused);
closure.close();
