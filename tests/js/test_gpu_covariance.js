'use strict';
// Covariance of the JavaScript front end on the GPU: the README Normal closure on 256 chains.  summarize(60, {window_rows: 4, covariance: true}) against a twin's
// sample(60) whose covariance is formed here, in JavaScript, in the restated order (per chain the Welford means and co-moments in row order; over the chains 256
// strided partial sums and a halving tree), compared within the cap L u (kappa_i + kappa_j) sd_i sd_j of tests/README.covariance.md; the twin's own covariance()
// over its stored draws is deep-equal to the summarised one; covariance() throws on a dataset sampler; dataset_covariance() answers per dataset with labels.
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
const C = 256, KEPT = 60;
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
// x, y [kept][chains] flat; x is the value with the smaller index.  diag: y === x and the whole-chain M2 takes the place of the co-moment
function restated(x, y, rows, chains) {
  const mx = new Float64Array(chains), my = new Float64Array(chains), w = new Float64Array(chains), diag = x === y;
  for (let c = 0; c < chains; c++) {
    let a = 0, b = 0, s = 0;
    for (let r = 0; r < rows; r++) {
      const k = r + 1, xv = x[r * chains + c], yv = y[r * chains + c];
      const dx = xv - a; a += dx / k;
      if (diag) { s += dx * (xv - a); continue; }
      const dy = yv - b; b += dy / k;
      s += dx * (yv - b);
    }
    mx[c] = a; my[c] = diag ? a : b; w[c] = s;
  }
  const gi = treeSum(strided(mx)) / chains, gj = treeSum(strided(my)) / chains, within = treeSum(strided(w));
  const between = treeSum(strided(Float64Array.from(mx, (m, c) => (m - gi) * (my[c] - gj))));
  return (within + rows * between) / (rows * chains - 1);
}

const folded = make({}), stored = make({}), host = make({});
for (const s of [folded, stored, host]) s.burn(150);
const draws = host.sample(KEPT);
assert.strictEqual(stored.sample_on_device(KEPT), KEPT);
assert.strictEqual(folded.summarize(KEPT, { window_rows: 4, covariance: true }), KEPT);
const got = folded.covariance(), twin = stored.covariance();
assert.deepStrictEqual(got.labels, ['mu', 'sigma']);
assert.deepStrictEqual(got, twin, 'the summarised matrix equals the stored one');
assert.deepStrictEqual(folded.dataset_covariance(), [got]);
const cols = [draws.mu, draws.sigma], U = Math.pow(2, -53), L = KEPT + C / 256 + 8;
const sd = cols.map((x) => Math.sqrt(restated(x, x, KEPT, C)));
const kappa = cols.map((x, i) => 1 + x.reduce((m, v) => Math.max(m, Math.abs(v)), 0) / sd[i]);
for (let i = 0; i < 2; i++) for (let j = 0; j < 2; j++) {
  const want = i === j ? restated(cols[i], cols[i], KEPT, C) : restated(cols[0], cols[1], KEPT, C);
  const cap = L * U * (kappa[i] + kappa[j]) * sd[i] * sd[j];
  assert.ok(Math.abs(got.cov[i][j] - want) <= cap, 'cov[' + i + '][' + j + ']: ' + got.cov[i][j] + ' against ' + want + ' (cap ' + cap + ')');
}
assert.strictEqual(got.cov[0][1], got.cov[1][0]);
assert.deepStrictEqual(got.cor, mcmc.correlation(got.cov));
assert.ok(got.cor[0][0] === 1 && got.cor[1][1] === 1 && Math.abs(got.cor[0][1]) < 1);
const m = folded.moments();
assert.strictEqual(Math.sqrt(got.cov[0][0]), m.mu.sd[0]);
assert.strictEqual(Math.sqrt(got.cov[1][1]), m.sigma.sd[0]);
// names: a subset in another order permutes the matrix
const rev = stored.covariance(['sigma', 'mu']);
assert.deepStrictEqual(rev.labels, ['sigma', 'mu']);
assert.deepStrictEqual(rev.cov, [[twin.cov[1][1], twin.cov[1][0]], [twin.cov[0][1], twin.cov[0][0]]]);
assert.deepStrictEqual(stored.covariance(['sigma']).cov, [[twin.cov[1][1]]]);
assert.throws(() => stored.covariance(['tau']), (e) => typeof e === 'string' && /tau/.test(e));
// a summarising call without a covariance folds none: the library's refusal names amwg_set_covariance; names afterwards are refused too
folded.summarize(KEPT, { window_rows: 4 });
assert.throws(() => folded.covariance(), (e) => /amwg_set_covariance/.test(String(e && e.message ? e.message : e)));
folded.summarize(KEPT, { window_rows: 4, covariance: ['sigma', 'mu'] });
assert.deepStrictEqual(folded.covariance().labels, ['sigma', 'mu']);
assert.throws(() => folded.covariance(['mu']), (e) => /amwg_set_covariance/.test(String(e && e.message ? e.message : e)));
// a storing call after the armed one: covariance() answers from the stored draws again, over every value or any names
folded.sample_on_device(KEPT);
assert.deepStrictEqual(folded.covariance().labels, ['mu', 'sigma']);
assert.deepStrictEqual(folded.covariance(['mu']).cov, [[folded.covariance().cov[0][0]]]);
for (const s of [folded, stored, host]) s.close();

// a dataset sampler: covariance() pools all chains and throws; dataset_covariance() answers per dataset
{
  const sets = [data, data.map((x) => x - 20), data.map((x) => x + 15)];
  const ds = new mcmc.AmwgSampler(params, log_post, null, { datasets: sets, chains: 3 * 64, seed: 20261020, lanes_per_chain: 1, block_threads: 64 });
  ds.burn(150);
  ds.sample_on_device(20);
  assert.throws(() => ds.covariance(), (e) => /pools all chains|pooled summaries are refused/.test(String(e && e.message ? e.message : e)));
  const per = ds.dataset_covariance();
  assert.strictEqual(per.length, 3);
  for (const o of per) {
    assert.deepStrictEqual(o.labels, ['mu', 'sigma']);
    assert.ok(o.cov[0][0] > 0 && o.cov[1][1] > 0 && o.cov[0][1] === o.cov[1][0] && Math.abs(o.cor[0][1]) <= 1);
  }
  ds.summarize(20, { window_rows: 3, covariance: ['mu'] });
  assert.strictEqual(ds.dataset_covariance().length, 3);
  ds.close();
}
console.log('gpu covariance ok');
