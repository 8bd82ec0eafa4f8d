'use strict';
// dataset_waic() and waic() of the JavaScript front end on the GPU: the README Normal closure on three datasets x 64 chains in ONE sampler (options.datasets).
// One entry per dataset -- elpd_waic, se, p_waic, lppd, waic, high_variance, pointwise -- against the rule of include/amwg.h restated here over that dataset's slice
// of the array sample() returned: the terms by this process's own ld.norm (V8's Math.log, which the device restates), lppd_i and p_i by compensated sums, within the
// header's bounds (u = 2^-53, E = 8 (S + 16) u); the totals from the returned pairs in index order, Object.is on every number.  The pooled waic() throws on the
// dataset sampler; after summarize() both throw the library's refusal; a translated closure is refused in the library's words; compare_waic on two fits.
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

const N = mcmc.native(), D = 3, CPD = 64, SEED = 20261021, NOBS = [40, 75, 50], KEPT = 14, U = Math.pow(2, -53);
const datasets = [];
for (let d = 0; d < D; d++) {      // seeded synthetic heights: sums of twelve Philox uniforms around a mean that differs per dataset
  const x = [];
  for (let i = 0; i < NOBS[d]; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(950 + d, 1, i * 12 + k); x.push(170 + 5 * d + 7 * (s - 6)); }
  datasets.push(x);
}
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(200); s.thin(3); return s.sample(40); }
const message = (e) => String(e && e.message ? e.message : e);

// a sum whose error does not grow with its length (Neumaier)
function csum(n, f) {
  let s = 0, c = 0;
  for (let k = 0; k < n; k++) { const v = f(k), t = s + v; c += Math.abs(s) >= Math.abs(v) ? (s - t) + v : (v - t) + s; s = t; }
  return s + c;
}
// the rule for one observation under the draws (mu[s], sigma[s]) -> [lppd_i, p_i, mean, max |l|]
function pair(x, mu, sigma) {
  const S = mu.length, l = new Float64Array(S);
  let m = -Infinity, big = 0;
  for (let s = 0; s < S; s++) { l[s] = ld.norm(x, mu[s], sigma[s]); m = Math.max(m, l[s]); big = Math.max(big, Math.abs(l[s])); }
  const lppd = m + Math.log(csum(S, (s) => Math.exp(l[s] - m))) - Math.log(S);
  const mean = csum(S, (s) => l[s]) / S;
  return [lppd, csum(S, (s) => (l[s] - mean) * (l[s] - mean)) / (S - 1), mean, big];
}
function totals(pw) {
  const n = pw.length;
  let lppd = 0, p = 0, elpd = 0, high = 0, ss = 0;
  for (let i = 0; i < n; i++) { lppd += pw[i][0]; p += pw[i][1]; elpd += pw[i][0] - pw[i][1]; if (pw[i][1] > 0.4) high++; }
  for (let i = 0; i < n; i++) { const e = (pw[i][0] - pw[i][1]) - elpd / n; ss += e * e; }
  return { elpd_waic: elpd, se: Math.sqrt(n * ss / (n - 1)), p_waic: p, lppd, waic: -2 * elpd, high_variance: high };
}
function check(entry, x, mu, sigma) {
  const S = mu.length, E = 8 * (S + 16) * U;
  assert.deepStrictEqual(Object.keys(entry), ['elpd_waic', 'se', 'p_waic', 'lppd', 'waic', 'high_variance', 'pointwise']);
  assert.strictEqual(entry.pointwise.length, x.length);
  let worst = 0;
  x.forEach((xi, i) => {
    const [lppd, p, mean, big] = pair(xi, mu, sigma), got = entry.pointwise[i];
    const rl = Math.abs(got[0] - lppd) / (E + 4 * U * Math.abs(lppd)), rp = Math.abs(got[1] - p) / (E * Math.sqrt(p * (p + mean * mean)) + (E * big) * (E * big));
    worst = Math.max(worst, rl, rp);
    assert.ok(rl <= 1 && rp <= 1, 'observation ' + i + ': ' + rl + ' ' + rp);
  });
  const want = totals(entry.pointwise);
  for (const k of Object.keys(want)) assert.ok(Object.is(entry[k], want[k]), k + ': ' + entry[k] + ' vs ' + want[k]);
  return worst;
}

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets, chains: D * CPD }, common));
assert.throws(() => all.dataset_waic(), (e) => /amwg_last_sample_dataset_waic/.test(message(e)) && /no sample\(\) call yet/.test(message(e)));
const got = run(all);
assert.strictEqual(got.mu.layout.kept, KEPT);
const dw = all.dataset_waic({ pointwise: true }), plain = all.dataset_waic();
assert.strictEqual(dw.length, D);
for (let d = 0; d < D; d++) {
  const mu = new Float64Array(KEPT * CPD), sigma = new Float64Array(KEPT * CPD);      // this dataset's slice of sample()'s [kept][chains], draw s = row * CPD + chain
  for (let t = 0; t < KEPT; t++) {
    mu.set(got.mu.subarray(t * D * CPD + d * CPD, t * D * CPD + (d + 1) * CPD), t * CPD);
    sigma.set(got.sigma.subarray(t * D * CPD + d * CPD, t * D * CPD + (d + 1) * CPD), t * CPD);
  }
  const worst = check(dw[d], datasets[d], mu, sigma);
  console.log('dataset ' + d + ' (n = ' + NOBS[d] + '): elpd ' + dw[d].elpd_waic.toFixed(3) + ' +- ' + dw[d].se.toFixed(3) + ', p_waic ' + dw[d].p_waic.toFixed(3) + ', largest error / bound ' + worst.toExponential(2));
  assert.ok(!('pointwise' in plain[d]));
  for (const k of Object.keys(plain[d])) assert.ok(Object.is(plain[d][k], dw[d][k]), k);
}
assert.throws(() => all.waic(), (e) => /datasets/.test(message(e)));
all.summarize(40);
const refusal = (e) => /amwg_last_sample_dataset_waic/.test(message(e)) && /amwg_sample_summarize/.test(message(e));
assert.throws(() => all.dataset_waic(), refusal);
all.close();

// ordinary samplers: waic() is the one entry of dataset_waic(); two fits of the same observations compared
const fit = (seed) => { const s = new mcmc.AmwgSampler(params, log_post, datasets[1], Object.assign({}, common, { seed, chains: CPD })); run(s); return s; };
const a = fit(SEED), b = fit(SEED + 1);
const wa = a.waic({ pointwise: true }), wb = b.waic({ pointwise: true });
assert.deepStrictEqual(a.dataset_waic({ pointwise: true }), [wa]);
const cmp = mcmc.compare_waic(wa, wb), self = mcmc.compare_waic(wa, wa);
assert.deepStrictEqual(self, { elpd_diff: 0, se_diff: 0 });
assert.ok(Math.abs(cmp.elpd_diff - (wa.elpd_waic - wb.elpd_waic)) <= 1e-10 && cmp.se_diff >= 0 && Math.abs(cmp.elpd_diff) < 1);      // two runs of one model: the same fit
assert.throws(() => mcmc.compare_waic(wa, dw[0]), (e) => /not the same data/.test(message(e)));
a.summarize(20);
assert.throws(() => a.waic(), refusal);
a.close();
b.close();

// a translated closure: its pointwise terms are not known to the library
const tr = new mcmc.AmwgSampler(params, log_post, datasets[0], Object.assign({}, common, { chains: CPD, translate: true }));
tr.burn(50);
tr.sample(10);
assert.throws(() => tr.waic(), (e) => /amwg_last_sample_dataset_waic/.test(message(e)) && /the pointwise terms of a closure are not known to the library; built-in families only/.test(message(e)));
tr.close();
console.log('gpu waic ok');
