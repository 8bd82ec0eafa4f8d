'use strict';
// Histograms of the JavaScript front end on the GPU: the README Normal closure on 256 chains.  summarize(60, {window_rows: 4, histogram}) against a twin's sample(60)
// binned in JavaScript by the rule itself (edges[i] <= x < edges[i + 1]): the counts are deep-equal -- integers, no tolerance --, and equal to the twin's own
// histogram(edges) over its stored draws; the twin's quantiles() lie inside interval_brackets() of the summarised counts; histogram() throws on a dataset sampler;
// dataset_histogram() without an armed histogram throws the library's refusal.
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
const make = (extra) => new mcmc.AmwgSampler(params, log_post, data, Object.assign({ chains: 256, seed: 20261019 }, extra));

// the rule, by linear search: [c_0 .. c_{bins-1}, under, over, nan]
function bin(values, edges) {
  const bins = edges.length - 1, c = new Array(bins + 3).fill(0);
  for (const x of values) {
    if (x !== x) c[bins + 2]++;
    else if (x < edges[0]) c[bins]++;
    else if (x >= edges[bins]) c[bins + 1]++;
    else { let i = 0; while (!(edges[i] <= x && x < edges[i + 1])) i++; c[i]++; }
  }
  return c;
}

const stored = make({}), folded = make({}), host = make({});
for (const s of [stored, folded, host]) s.burn(150);
const draws = host.sample(60);
assert.strictEqual(stored.sample_on_device(60), 60);
const BINS = 48, edges = {};
for (const name of ['mu', 'sigma']) {
  let lo = Infinity, hi = -Infinity;
  for (const x of draws[name]) { lo = Math.min(lo, x); hi = Math.max(hi, x); }
  const w = (hi - lo) / (BINS - 2);      // the draws' own range widened by one bin either side: every rank falls into a real bin
  edges[name] = Array.from({ length: BINS + 1 }, (_, i) => lo - w + i * w);
}
assert.strictEqual(folded.summarize(60, { window_rows: 4, histogram: edges }), 60);
const got = folded.histogram(), twin = stored.histogram(edges), q = stored.quantiles([0.025, 0.5, 0.975]);
assert.deepStrictEqual(Object.keys(got), ['mu', 'sigma']);
for (const name of ['mu', 'sigma']) {
  const want = bin(draws[name], edges[name]);
  assert.strictEqual(got[name].length, 1);
  assert.deepStrictEqual(got[name][0], want, name + ': summarised counts');
  assert.deepStrictEqual(twin[name][0], want, name + ': stored counts');
  assert.strictEqual(want.reduce((a, b) => a + b, 0), 60 * 256);
  assert.deepStrictEqual(want.slice(BINS), [0, 0, 0]);
  const br = mcmc.interval_brackets(got[name][0], edges[name], [0.025, 0.5, 0.975]), w = edges[name][1] - edges[name][0];
  br.forEach(([lo, hi], k) => {
    assert.ok(lo <= q[name][0][k] && q[name][0][k] <= hi, name + ' quantile ' + k + ': ' + lo + ' <= ' + q[name][0][k] + ' <= ' + hi);
    assert.ok(hi - lo <= 2 * w * (1 + 1e-9));
  });
}
assert.deepStrictEqual(folded.dataset_histogram(), [got]);
// one array of edges for all values
const both = Array.from({ length: 11 }, (_, i) => 20 * i);
const shared = stored.histogram(both);
assert.deepStrictEqual(shared.mu[0], bin(draws.mu, both));
assert.deepStrictEqual(shared.sigma[0], bin(draws.sigma, both));
// interval_brackets by hand: n = 10, ranks (0, 1), (4, 5), (9, 9); a counted NaN; ranks in under / over
assert.deepStrictEqual(mcmc.interval_brackets([3, 4, 2, 1, 0, 0, 0], [0, 1, 2.5, 4, 8], [0, 0.5, 1]), [[0, 1], [1, 2.5], [4, 8]]);
assert.deepStrictEqual(mcmc.interval_brackets([3, 4, 2, 1, 0, 0, 1], [0, 1, 2.5, 4, 8], [0.5, 2]), [[NaN, NaN], [NaN, NaN]]);
assert.deepStrictEqual(mcmc.interval_brackets([2, 2, 2, 2, 6, 0, 0], [0, 1, 2.5, 4, 8], [0, 1]), [[-Infinity, 0], [4, 8]]);
assert.deepStrictEqual(mcmc.interval_brackets([2, 2, 2, 2, 0, 6, 0], [0, 1, 2.5, 4, 8], [0, 1]), [[0, 1], [8, Infinity]]);
// a summarising call without a histogram counts nothing: the library's refusal names amwg_set_histogram; bad edges are refused
folded.summarize(60, { window_rows: 4 });
assert.throws(() => folded.histogram(), (e) => /amwg_set_histogram/.test(String(e && e.message ? e.message : e)));
assert.throws(() => stored.histogram({ mu: [0, 1, 1], sigma: [0, 1, 2] }), (e) => /strictly ascending/.test(String(e && e.message ? e.message : e)));
assert.throws(() => stored.histogram({ mu: [0, 1, 2] }), (e) => typeof e === 'string' && /sigma/.test(e));
for (const s of [stored, folded, host]) s.close();

// a dataset sampler: histogram() pools all chains and throws; dataset_histogram() answers per dataset
{
  const sets = [data, data.map((x) => x - 20), data.map((x) => x + 15)];
  const ds = new mcmc.AmwgSampler(params, log_post, null, { datasets: sets, chains: 3 * 64, seed: 20261019, lanes_per_chain: 1, block_threads: 64 });
  ds.burn(150);
  ds.sample_on_device(20);
  assert.throws(() => ds.histogram(both), (e) => /pools all chains|pooled summaries are refused/.test(String(e && e.message ? e.message : e)));
  const per = ds.dataset_histogram(Array.from({ length: 41 }, (_, i) => 10 * i));
  assert.strictEqual(per.length, 3);
  for (const o of per) assert.strictEqual(o.mu[0].reduce((a, b) => a + b, 0), 20 * ds.chains_per_dataset);
  ds.close();
}
console.log('gpu histogram ok');
