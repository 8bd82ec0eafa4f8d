'use strict';
// dataset_waic({groups}), dataset_loo({groups}), waic({groups}), loo({groups}) and both compare_* of the JavaScript front end on the GPU -- leave-one-group-out
// (include/amwg.h): the README Normal closure on three ragged datasets x 64 chains in ONE sampler, each dataset with a label array of its own (unsorted, not dense).
// WAIC per group against the rule restated over sample()'s draws: the joint term is the left-to-right sum of the members' ld.norm in ascending observation index,
// lppd_g and p_g within the bounds of the header; the totals from the returned pairs in group order (Object.is).  LOO per group: lppd_g is dataset_waic({groups})'s
// own number, the totals follow from the triples.  Singleton groups return the ungrouped pointwise values.  compare_* throw when the group counts differ.
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

const N = mcmc.native(), D = 3, CPD = 64, SEED = 20261126, NOBS = [40, 75, 50], NG = [4, 9, 1], KEPT = 14, U = Math.pow(2, -53);
const datasets = [], groups = [];
for (let d = 0; d < D; d++) {
  const x = [], g = [];
  for (let i = 0; i < NOBS[d]; i++) {
    let s = 0;
    for (let k = 0; k < 12; k++) s += N.uniform(960 + d, 1, i * 12 + k);
    x.push(170 + 5 * d + 7 * (s - 6));
    g.push(100 - 7 * ((i * 5 + d) % NG[d]));      // labels in no order, multiples of 7 downwards from 100
  }
  datasets.push(x);
  groups.push(d === 1 ? Int32Array.from(g) : g);
}
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(200); s.thin(3); return s.sample(40); }
const message = (e) => String(e && e.message ? e.message : e);
function csum(n, f) {      // Neumaier
  let s = 0, c = 0;
  for (let k = 0; k < n; k++) { const v = f(k), t = s + v; c += Math.abs(s) >= Math.abs(v) ? (s - t) + v : (v - t) + s; s = t; }
  return s + c;
}
// the groups of a label array: the distinct labels ascending, each with its members in ascending observation index
const members = (g) => Array.from(new Set(g)).sort((a, b) => a - b).map((name) => Array.from(g.keys()).filter((i) => g[i] === name));
function waic_totals(pw) {
  const n = pw.length;
  let lppd = 0, p = 0, elpd = 0, high = 0, ss = 0;
  for (let i = 0; i < n; i++) { lppd += pw[i][0]; p += pw[i][1]; elpd += pw[i][0] - pw[i][1]; if (pw[i][1] > 0.4) high++; }
  for (let i = 0; i < n; i++) { const e = (pw[i][0] - pw[i][1]) - elpd / n; ss += e * e; }
  return { elpd_waic: elpd, se: Math.sqrt(n * ss / (n - 1)), p_waic: p, lppd, waic: -2 * elpd, high_variance: high };
}
function loo_totals(pw) {
  const n = pw.length;
  let elpd = 0, lppd = 0, high = 0, ss = 0;
  for (let i = 0; i < n; i++) { elpd += pw[i][0]; lppd += pw[i][1]; if (pw[i][2] > 0.7) high++; }
  for (let i = 0; i < n; i++) { const e = pw[i][0] - elpd / n; ss += e * e; }
  return { elpd_loo: elpd, se: Math.sqrt(n * ss / (n - 1)), p_loo: lppd - elpd, lppd, looic: -2 * elpd, high_k: high };
}

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets, chains: D * CPD }, common));
const got = run(all);
const gw = all.dataset_waic({ groups, pointwise: true }), gl = all.dataset_loo({ groups, pointwise: true }), plain = all.dataset_waic({ groups });
for (let d = 0; d < D; d++) {
  const S = KEPT * CPD, E = 8 * (S + 16) * U, sets = members(Array.from(groups[d]));
  assert.strictEqual(gw[d].n_groups, NG[d]);
  assert.strictEqual(gl[d].n_groups, NG[d]);
  assert.strictEqual(gw[d].pointwise.length, NG[d]);
  assert.ok(!('pointwise' in plain[d]) && Object.is(plain[d].elpd_waic, gw[d].elpd_waic));
  sets.forEach((set, g) => {
    const L = new Float64Array(S);
    let m = -Infinity, big = 0;
    for (let s = 0; s < S; s++) {
      const at = Math.floor(s / CPD) * D * CPD + d * CPD + s % CPD, mu = got.mu[at], sigma = got.sigma[at];
      let acc = ld.norm(datasets[d][set[0]], mu, sigma);
      for (let k = 1; k < set.length; k++) acc = acc + ld.norm(datasets[d][set[k]], mu, sigma);
      L[s] = acc; m = Math.max(m, acc); big = Math.max(big, Math.abs(acc));
    }
    const lppd = m + Math.log(csum(S, (s) => Math.exp(L[s] - m))) - Math.log(S), mean = csum(S, (s) => L[s]) / S, p = csum(S, (s) => (L[s] - mean) * (L[s] - mean)) / (S - 1);
    const pair = gw[d].pointwise[g];
    const rl = Math.abs(pair[0] - lppd) / (E + 4 * U * Math.abs(lppd)), rp = Math.abs(pair[1] - p) / (E * Math.sqrt(p * (p + mean * mean)) + (E * big) * (E * big));
    assert.ok(rl <= 1 && rp <= 1, 'dataset ' + d + ' group ' + g + ': error / bound ' + rl + ' ' + rp);
    assert.ok(Object.is(gl[d].pointwise[g][1], pair[0]), 'lppd_g of loo');
    assert.ok(Number.isFinite(gl[d].pointwise[g][0]) && gl[d].pointwise[g][0] <= pair[0] + 0.05, 'elpd_loo_g beside lppd_g');
  });
  const ww = waic_totals(gw[d].pointwise), wl = loo_totals(gl[d].pointwise);
  for (const k of Object.keys(ww)) assert.ok(Object.is(gw[d][k], ww[k]) || (NG[d] === 1 && k === 'se' && Number.isNaN(gw[d][k])), k + ': ' + gw[d][k] + ' vs ' + ww[k]);
  for (const k of Object.keys(wl)) assert.ok(Object.is(gl[d][k], wl[k]) || (NG[d] === 1 && k === 'se' && Number.isNaN(gl[d][k])), k + ': ' + gl[d][k] + ' vs ' + wl[k]);
  console.log('dataset ' + d + ': ' + NG[d] + ' groups of ' + NOBS[d] + ' observations, elpd_waic ' + gw[d].elpd_waic.toFixed(3) + ', elpd_loo ' + gl[d].elpd_loo.toFixed(3));
}
assert.throws(() => all.dataset_waic({ groups: groups.slice(1) }), (e) => /one array of labels per dataset/.test(message(e)));
assert.throws(() => all.dataset_loo({ groups: [groups[0], groups[1], groups[2].slice(1)] }), (e) => /one label per observation/.test(message(e)));
assert.throws(() => mcmc.compare_waic(gw[0], gw[1]), (e) => /4 groups and 9 groups/.test(message(e)));
assert.throws(() => mcmc.compare_loo(gl[0], gl[1]), (e) => /4 groups and 9 groups/.test(message(e)));
all.close();

// an ordinary sampler: waic({groups}) / loo({groups}) take the one label array; singleton groups are the ungrouped values; grouped and ungrouped do not compare
const one = new mcmc.AmwgSampler(params, log_post, datasets[0], Object.assign({}, common, { chains: CPD }));
run(one);
const w = one.waic({ pointwise: true }), l = one.loo({ pointwise: true }), singles = Array.from({ length: NOBS[0] }, (_, i) => i);
const ws = one.waic({ groups: singles, pointwise: true }), ls = one.loo({ groups: Int32Array.from(singles), pointwise: true }), w4 = one.waic({ groups: groups[0], pointwise: true });
assert.deepStrictEqual(ws.pointwise, w.pointwise);
assert.deepStrictEqual(ls.pointwise, l.pointwise);
assert.strictEqual(ws.n_groups, NOBS[0]);
assert.deepStrictEqual(mcmc.compare_waic(w4, w4), { elpd_diff: 0, se_diff: 0 });
assert.throws(() => mcmc.compare_waic(w, w4), (e) => /observations and 4 groups/.test(message(e)));
assert.throws(() => mcmc.compare_loo(ls, one.loo({ groups: groups[0], pointwise: true })), (e) => /40 groups and 4 groups/.test(message(e)));
one.summarize(20);
assert.throws(() => one.loo({ groups: singles }), (e) => /amwg_last_sample_dataset_loo_grouped/.test(message(e)) && /amwg_sample_summarize/.test(message(e)));
one.close();
console.log('gpu grouped ok');
