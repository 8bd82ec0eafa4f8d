'use strict';
// summarize() of the JavaScript front end on the GPU: the README Normal closure on 256 chains, and the closure of examples/hierarchical_binomial.js (translated, with
// a derived quantity: more recorded values than parameters).  summarize(60, {window_rows: 4}) against a twin's sample_on_device(60): convergence() deep-equal (the
// accumulated halves are the stored halves, bit for bit), moments() within 4 N u S of the moments of the draws themselves (a third twin's sample(60): the same draws;
// Neumaier-compensated sums, whose own error is a few u S), quantiles() throws the library's refusal, and a sampler on two shards throws at summarize().
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;

const U = Math.pow(2, -53);
function neumaier(n, f) {
  let s = 0, c = 0;
  for (let i = 0; i < n; i++) { const v = f(i), t = s + v; c += Math.abs(s) >= Math.abs(v) ? (s - t) + v : (v - t) + s; s = t; }
  return s + c;
}

function check(name, make) {
  const stored = make({}), folded = make({}), host = make({});
  for (const s of [stored, folded, host]) s.burn(150);
  assert.strictEqual(stored.sample_on_device(60), 60);
  assert.strictEqual(folded.summarize(60, { window_rows: 4 }), 60);
  const draws = host.sample(60);
  const si = folded.summary_info(), C = folded.chains;
  assert.strictEqual(si.rows, 60);
  assert.strictEqual(si.window_rows, 4);
  assert.strictEqual(si.windows, 15);
  assert.strictEqual(si.window_bytes, 4 * folded.PR * C * 8);
  assert.strictEqual(si.accumulator_bytes, 6 * folded.PR * C * 8);
  assert.deepStrictEqual(folded.convergence(), stored.convergence());
  const mom = folded.moments(), ref = stored.moments();
  assert.deepStrictEqual(Object.keys(mom), Object.keys(ref));
  assert.ok(Object.keys(mom).length > 0);
  let checked = 0;
  for (const key of Object.keys(mom)) {
    const arr = draws[key], len = mom[key].mean.length, n = 60 * C;
    assert.ok(arr && arr.length === n * len, name + ': sample() returns ' + key);
    for (let e = 0; e < len; e++) {
      const at = (i) => arr[(Math.floor(i / C) * len + e) * C + (i % C)];
      let S = 0;
      for (let i = 0; i < n; i++) S = Math.max(S, Math.abs(at(i)));
      const mean = neumaier(n, at) / n, sd = Math.sqrt(neumaier(n, (i) => (at(i) - mean) * (at(i) - mean)) / (n - 1)), bound = 4 * n * U * S;
      assert.ok(Math.abs(mom[key].mean[e] - mean) <= bound, name + ' mean of ' + key + '[' + e + ']: ' + mom[key].mean[e] + ' vs ' + mean);
      assert.ok(Math.abs(mom[key].sd[e] - sd) <= bound, name + ' sd of ' + key + '[' + e + ']: ' + mom[key].sd[e] + ' vs ' + sd);
      checked++;
    }
  }
  assert.strictEqual(checked, folded.PR);
  const refusal = (e) => /amwg_sample_summarize/.test(String(e && e.message ? e.message : e));
  assert.throws(() => folded.quantiles([0.5]), refusal);
  assert.throws(() => folded.dataset_quantiles([0.5]), refusal);
  assert.ok(stored.quantiles([0.5]));
  // the next sample call replaces the summary
  folded.sample_on_device(8);
  assert.ok(folded.quantiles([0.5]));
  assert.throws(() => folded.summary_info(), (e) => /amwg_summary_info/.test(String(e && e.message ? e.message : e)));
  for (const s of [stored, folded, host]) s.close();
  const two = make({ devices: [0, 0] });
  assert.throws(() => two.summarize(60, { window_rows: 4 }), (e) => typeof e === 'string' && /several devices/.test(e) && /stored draws/.test(e));
  two.close();
  const one = make({});
  assert.throws(() => one.summarize(60, { devices: [0, 1] }), (e) => typeof e === 'string' && /several devices/.test(e));
  one.close();
}

// the README program's model
{
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
  check('readme normal', (extra) => new mcmc.AmwgSampler(params, log_post, data, Object.assign({ chains: 256, seed: 20261018 }, extra)));
}

// the closure of examples/hierarchical_binomial.js: translated, and its derived quantity mean_p is recorded after the eight parameters' components
{
  const binom_data = { x: [5, 6, 9, 14, 13, 20], n: [10, 10, 20, 20, 30, 30] };
  const params = {
    p: { type: 'real', init: 0.5, lower: 0, upper: 1, dim: [1, 6] },
    mu_logit_p: { type: 'real', init: 0 },
    sigma_logit_p: { type: 'real', lower: 0, init: 1 } };
  const logit = function (p) { return Math.log(p / (1 - p)); };
  const log_post = function (par, d) {
    var p = par.p[0];
    var mu_logit_p = par.mu_logit_p;
    var sigma_logit_p = par.sigma_logit_p;
    var log_post = 0;
    log_post += ld.norm(mu_logit_p, 0, 10);
    log_post += ld.norm(sigma_logit_p, 0, 10);
    for (var i = 0; i < d.x.length; i++) {
      log_post += ld.norm(logit(p[i]), mu_logit_p, sigma_logit_p);
      log_post += ld.binom(d.x[i], d.n[i], p[i]);
    }
    par.mean_p = (p[0] + p[1] + p[2] + p[3] + p[4] + p[5]) / 6;
    return log_post;
  };
  global.logit = logit;
  const made = [];
  check('hierarchical binomial', (extra) => { const s = new mcmc.AmwgSampler(params, log_post, binom_data, Object.assign({ helpers: { logit: logit }, chains: 256, seed: 7 }, extra)); made.push(s); return s; });
  assert.ok(made[0].PR > made[0].P && made[0].derived.indexOf('mean_p') >= 0);
}
console.log('gpu summarize ok');
