'use strict';
// Autocorrelation of the JavaScript front end on the GPU: the README Normal closure on 256 chains.  summarize(60, {window_rows: 4, autocorrelation: {max_lag: 6}})
// against a twin's sample(60) whose autocovariance is formed here, in JavaScript, in the restated order of include/amwg.h (per chain the lag sums about the pilot
// in row order and the finish; over the chains 256 strided partial sums and a halving tree): the same doubles.  The twin's own autocorrelation() over its stored
// draws is deep-equal to the summarised one; autocorrelation() throws on a dataset sampler; dataset_autocorrelation() answers per dataset with labels.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;

const data = [183, 192, 182, 183, 177, 185, 188, 188, 182, 185];
const params = { mu: { type: 'real' }, sigma: { type: 'real', lower: 0 } };
const log_post = function (state, data) {
  var log_post = 0;
  log_post += ld.norm(state.mu, 0, 100);
  log_post += ld.unif(state.sigma, 0, 100);
  for (var i = 0; i < data.length; i++) {
    log_post += ld.norm(data[i], state.mu, state.sigma);
  }
  return log_post;
};
const C = 256, KEPT = 60, LAG = 6;
const make = (extra) => new mcmc.AmwgSampler(params, log_post, data, Object.assign({ chains: C, seed: 20261020 }, extra));

function treeSum(partial) {      // the halving tree over 256 partial sums
  const red = Float64Array.from(partial);
  for (let o = red.length >> 1; o > 0; o >>= 1) for (let t = 0; t < o; t++) red[t] += red[t + o];
  return red[0];
}
function strided(v) {      // thread t sums v[t], v[t + 256], ...
  const acc = new Float64Array(256);
  for (let i = 0; i < v.length; i++) acc[i % 256] += v[i];
  return acc;
}
// x [kept][chains] flat -> {acov [L + 1], between}
function restated(x, n, chains, L) {
  const gamma = Array.from({ length: L + 1 }, () => new Float64Array(chains)), m = new Float64Array(chains);
  for (let c = 0; c < chains; c++) {
    const a = x[c], y = new Float64Array(n), S = new Float64Array(L + 1);
    let Y = 0;
    for (let t = 0; t < n; t++) {
      y[t] = x[t * chains + c] - a;
      Y += y[t];
      for (let l = 0; l <= Math.min(t, L); l++) S[l] += y[t] * y[t - l];
    }
    const yb = Y / n;
    let H = 0, T = 0;
    for (let l = 0; l <= L; l++) {
      gamma[l][c] = ((S[l] - yb * ((Y - H) + (Y - T))) + (n - l) * (yb * yb)) / n;
      if (l < L) { H += y[l]; T += y[n - 1 - l]; }
    }
    m[c] = a + yb;
  }
  const acov = gamma.map((g) => treeSum(strided(g)) / chains);
  const gm = treeSum(strided(m)) / chains;
  const between = treeSum(strided(Float64Array.from(m, (v) => (v - gm) * (v - gm)))) / (chains - 1);
  return { acov, between };
}

const folded = make({}), stored = make({}), host = make({});
for (const s of [folded, stored, host]) s.burn(150);
const draws = host.sample(KEPT);
assert.strictEqual(stored.sample_on_device(KEPT), KEPT);
assert.strictEqual(folded.summarize(KEPT, { window_rows: 4, autocorrelation: { max_lag: LAG } }), KEPT);
const got = folded.autocorrelation(), twin = stored.autocorrelation(null, { max_lag: LAG });
assert.deepStrictEqual(got.labels, ['mu', 'sigma']);
assert.deepStrictEqual(got, twin, 'the summarised autocorrelation equals the stored one');
assert.deepStrictEqual(folded.dataset_autocorrelation(), [got]);
[draws.mu, draws.sigma].forEach((x, k) => {
  const want = restated(x, KEPT, C, LAG);
  assert.deepStrictEqual(got.acov[k], want.acov, 'acov of ' + got.labels[k] + ' in the restated order');
  const e = mcmc.autocorrelation_ess(want.acov, want.between, KEPT, C);
  assert.deepStrictEqual(got.rho[k], e.rho);
  assert.strictEqual(got.tau[k], e.tau);
  assert.strictEqual(got.ess[k], e.ess);
  assert.strictEqual(got.truncated[k], e.truncated);
  assert.ok(got.rho[k][0] === 1 && got.acov[k].length === LAG + 1 && got.tau[k] > 0.5 && got.ess[k] > 0);
});
// the default max_lag of a stored run: min(100, kept - 1)
assert.strictEqual(stored.autocorrelation().acov[0].length, KEPT);
// names: a subset in another order
const rev = stored.autocorrelation(['sigma', 'mu'], { max_lag: LAG });
assert.deepStrictEqual(rev.labels, ['sigma', 'mu']);
assert.deepStrictEqual(rev.acov, [twin.acov[1], twin.acov[0]]);
assert.throws(() => stored.autocorrelation(['tau']), (e) => typeof e === 'string' && /tau/.test(e));
// a summarising call without the option folds none: the library's refusal names amwg_set_autocovariance; names or lags afterwards are refused too
folded.summarize(KEPT, { window_rows: 4 });
assert.throws(() => folded.autocorrelation(), (e) => /amwg_set_autocovariance/.test(String(e && e.message ? e.message : e)));
folded.summarize(KEPT, { window_rows: 4, autocorrelation: { max_lag: 3, names: ['sigma'] } });
assert.deepStrictEqual(folded.autocorrelation().labels, ['sigma']);
assert.strictEqual(folded.autocorrelation().acov[0].length, 4);
assert.throws(() => folded.autocorrelation(['mu']), (e) => /amwg_set_autocovariance/.test(String(e && e.message ? e.message : e)));
assert.throws(() => folded.autocorrelation(null, { max_lag: 2 }), (e) => /amwg_set_autocovariance/.test(String(e && e.message ? e.message : e)));
// max_lag >= kept draws: the summarising call itself is refused
assert.throws(() => folded.summarize(KEPT, { autocorrelation: { max_lag: KEPT } }), (e) => /max_lag/.test(String(e && e.message ? e.message : e)));
// a storing call after the armed one: autocorrelation() answers from the stored draws again
folded.sample_on_device(KEPT);
assert.deepStrictEqual(folded.autocorrelation(['mu'], { max_lag: LAG }).labels, ['mu']);
for (const s of [folded, stored, host]) s.close();

// a dataset sampler: autocorrelation() pools all chains and throws; dataset_autocorrelation() answers per dataset
{
  const sets = [data, data.map((x) => x - 20), data.map((x) => x + 15)];
  const ds = new mcmc.AmwgSampler(params, log_post, null, { datasets: sets, chains: 3 * 64, seed: 20261020, lanes_per_chain: 1, block_threads: 64 });
  ds.burn(150);
  ds.sample_on_device(20);
  assert.throws(() => ds.autocorrelation(), (e) => /pools all chains|pooled summaries are refused/.test(String(e && e.message ? e.message : e)));
  const per = ds.dataset_autocorrelation(null, { max_lag: 5 });
  assert.strictEqual(per.length, 3);
  for (const o of per) {
    assert.deepStrictEqual(o.labels, ['mu', 'sigma']);
    assert.ok(o.acov[0][0] > 0 && o.acov[1][0] > 0 && o.rho[0][0] === 1 && o.acov[0].length === 6 && Number.isFinite(o.tau[0]) && Number.isFinite(o.ess[1]));
  }
  ds.summarize(20, { window_rows: 3, autocorrelation: { max_lag: 4, names: ['mu'] } });
  assert.strictEqual(ds.dataset_autocorrelation().length, 3);
  ds.close();
}
console.log('gpu autocorrelation ok');
