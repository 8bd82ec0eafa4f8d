'use strict';
// dataset_loo(), loo() and compare_loo of the JavaScript front end on the GPU: the README Normal closure on three datasets x 64 chains in ONE sampler
// (options.datasets).  One entry per dataset -- elpd_loo, se, p_loo, lppd, looic, high_k, pointwise -- whose lppd_i are dataset_waic()'s own numbers (Object.is),
// whose totals follow from the returned triples in index order (Object.is on every number), and whose elpd_loo_i lie just below their lppd_i, as they do for a
// well-specified model; the values themselves are pinned against the extended-precision reference by tests/test_gpu_loo.py.  elpd_loo and elpd_waic agree closely here.
// The pooled loo() throws on the dataset sampler; after summarize() both throw the library's refusal; a translated closure is refused in the library's words;
// compare_loo on two fits.
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

const N = mcmc.native(), D = 3, CPD = 64, SEED = 20261021, NOBS = [40, 75, 50], KEPT = 14;
const datasets = [];
for (let d = 0; d < D; d++) {      // seeded synthetic heights: sums of twelve Philox uniforms around a mean that differs per dataset
  const x = [];
  for (let i = 0; i < NOBS[d]; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(950 + d, 1, i * 12 + k); x.push(170 + 5 * d + 7 * (s - 6)); }
  datasets.push(x);
}
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(200); s.thin(3); return s.sample(40); }
const message = (e) => String(e && e.message ? e.message : e);

function totals(pw) {
  const n = pw.length;
  let elpd = 0, lppd = 0, high = 0, ss = 0;
  for (let i = 0; i < n; i++) { elpd += pw[i][0]; lppd += pw[i][1]; if (pw[i][2] > 0.7) high++; }
  for (let i = 0; i < n; i++) { const e = pw[i][0] - elpd / n; ss += e * e; }
  return { elpd_loo: elpd, se: Math.sqrt(n * ss / (n - 1)), p_loo: lppd - elpd, lppd, looic: -2 * elpd, high_k: high };
}

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets, chains: D * CPD }, common));
assert.throws(() => all.dataset_loo(), (e) => /amwg_last_sample_dataset_loo/.test(message(e)) && /no sample\(\) call yet/.test(message(e)));
const got = run(all);
assert.strictEqual(got.mu.layout.kept, KEPT);
const dl = all.dataset_loo({ pointwise: true }), plain = all.dataset_loo(), dw = all.dataset_waic({ pointwise: true });
assert.strictEqual(dl.length, D);
for (let d = 0; d < D; d++) {
  const e = dl[d];
  assert.deepStrictEqual(Object.keys(e), ['elpd_loo', 'se', 'p_loo', 'lppd', 'looic', 'high_k', 'pointwise']);
  assert.strictEqual(e.pointwise.length, NOBS[d]);
  e.pointwise.forEach((t, i) => {
    assert.strictEqual(t.length, 3);
    assert.ok(Object.is(t[1], dw[d].pointwise[i][0]), 'lppd_' + i);      // WAIC's own lppd_i
    assert.ok(Number.isFinite(t[0]) && t[0] <= t[1] + 0.05 && t[0] > t[1] - 5, 'elpd_loo_' + i + ' ' + t[0] + ' beside lppd ' + t[1]);
    assert.ok(t[2] === Infinity || (Number.isFinite(t[2]) && t[2] > -2 && t[2] < 5), 'khat_' + i + ' ' + t[2]);
  });
  const want = totals(e.pointwise);
  for (const k of Object.keys(want)) assert.ok(Object.is(e[k], want[k]), k + ': ' + e[k] + ' vs ' + want[k]);
  assert.ok(Object.is(e.lppd, dw[d].lppd));
  assert.ok(Math.abs(e.elpd_loo - dw[d].elpd_waic) < 0.02 * Math.abs(dw[d].elpd_waic) && e.p_loo > 0 && Math.abs(e.p_loo - dw[d].p_waic) < 0.02 * Math.abs(dw[d].elpd_waic),
            'elpd_loo ' + e.elpd_loo + ' elpd_waic ' + dw[d].elpd_waic + ' p_loo ' + e.p_loo + ' p_waic ' + dw[d].p_waic);      // the two estimates of one quantity: within 2 %
  console.log('dataset ' + d + ' (n = ' + NOBS[d] + '): elpd_loo ' + e.elpd_loo.toFixed(3) + ' +- ' + e.se.toFixed(3) + ', p_loo ' + e.p_loo.toFixed(3) + ', elpd_waic ' + dw[d].elpd_waic.toFixed(3) + ', p_waic ' + dw[d].p_waic.toFixed(3) +
              ', high_k ' + e.high_k);
  assert.ok(!('pointwise' in plain[d]));
  for (const k of Object.keys(plain[d])) assert.ok(Object.is(plain[d][k], e[k]), k);
}
assert.throws(() => all.loo(), (e) => /datasets/.test(message(e)));
all.summarize(40);
const refusal = (e) => /amwg_last_sample_dataset_loo/.test(message(e)) && /amwg_sample_summarize/.test(message(e));
assert.throws(() => all.dataset_loo(), refusal);
all.close();

// ordinary samplers: loo() is the one entry of dataset_loo(); two fits of the same observations compared
const fit = (seed) => { const s = new mcmc.AmwgSampler(params, log_post, datasets[1], Object.assign({}, common, { seed, chains: CPD })); run(s); return s; };
const a = fit(SEED), b = fit(SEED + 1);
const la = a.loo({ pointwise: true }), lb = b.loo({ pointwise: true });
assert.deepStrictEqual(a.dataset_loo({ pointwise: true }), [la]);
const cmp = mcmc.compare_loo(la, lb), self = mcmc.compare_loo(la, la);
assert.deepStrictEqual(self, { elpd_diff: 0, se_diff: 0 });
assert.ok(Math.abs(cmp.elpd_diff - (la.elpd_loo - lb.elpd_loo)) <= 1e-10 && cmp.se_diff >= 0 && Math.abs(cmp.elpd_diff) < 0.02 * Math.abs(la.elpd_loo),
          'elpd_diff ' + cmp.elpd_diff + ' se_diff ' + cmp.se_diff);      // two short runs of one model: the same fit within 2 % (a sanity check: the values are pinned in test_gpu_loo.py)
assert.throws(() => mcmc.compare_loo(la, dl[0]), (e) => /not the same data/.test(message(e)));
assert.throws(() => mcmc.compare_loo(la, a.loo()), (e) => /both results need pointwise/.test(message(e)));
a.summarize(20);
assert.throws(() => a.loo(), refusal);
a.close();
b.close();

// a translated closure: its pointwise terms are not known to the library
const tr = new mcmc.AmwgSampler(params, log_post, datasets[0], Object.assign({}, common, { chains: CPD, translate: true }));
tr.burn(50);
tr.sample(10);
assert.throws(() => tr.loo(), (e) => /amwg_last_sample_dataset_loo/.test(message(e)) && /the pointwise terms of a closure are not known to the library; built-in families only/.test(message(e)));
tr.close();
console.log('gpu loo ok');
