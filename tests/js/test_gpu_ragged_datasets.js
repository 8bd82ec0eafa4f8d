'use strict';
// options.datasets with UNEQUAL sizes on the GPU: the README Normal closure on three datasets of 5, 65 and 300 observations x 64 chains in ONE sampler.
// The front end picks the ragged entry by itself (amwg_create_datasets_ragged); layout.n_obs lists the sizes; each dataset's slice of sample() deep-equals a
// one-dataset sampler with chain_offset d * 64; dealing the datasets to two shards (devices: [0, 0]: datasets 0-1, of unequal sizes, and 2) returns the
// same draws.
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

const N = mcmc.native(), SIZES = [5, 65, 300], D = SIZES.length, CPD = 64, SEED = 20261018;
const datasets = [];
for (let d = 0; d < D; d++) {      // seeded synthetic heights: sums of twelve Philox uniforms around a mean that differs per dataset
  const x = [];
  for (let i = 0; i < SIZES[d]; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(950 + d, 1, i * 12 + k); x.push(170 + 5 * d + 7 * (s - 6)); }
  datasets.push(x);
}
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(120); s.thin(3); return s.sample(40); }

const all = new mcmc.AmwgSampler(params, log_post, null, Object.assign({ datasets, chains: D * CPD }, common));
const got = run(all);
assert.deepStrictEqual(got.mu.layout, { kept: 14, len: 1, chains: D * CPD, dim: [1], datasets: D, chains_per_dataset: CPD });
assert.deepStrictEqual(got.mu.layout.n_obs, SIZES);      // (not enumerable: the layout of a dataset sampler lists what it always did)
assert.deepStrictEqual(got.sigma.layout.n_obs, SIZES);
assert.ok(all.info().launch[0].kernel.indexOf('_ds<') > 0 && all.info().launch[0].datasets === D);
const slice = (arr, d) => { const o = []; for (let t = 0; t < 14; t++) o.push(Array.from(arr.subarray(t * D * CPD + d * CPD, t * D * CPD + (d + 1) * CPD))); return o; };
const dm = all.dataset_moments();
assert.strictEqual(dm.length, D);
for (let d = 0; d < D; d++) {
  const one = new mcmc.AmwgSampler(params, log_post, datasets[d], Object.assign({ chains: CPD, chain_offset: d * CPD }, common));
  const want = run(one);
  for (const name of ['mu', 'sigma']) {
    const w = []; for (let t = 0; t < 14; t++) w.push(Array.from(want[name].subarray(t * CPD, (t + 1) * CPD)));
    assert.deepStrictEqual(slice(got[name], d), w, 'dataset ' + d + ' ' + name);
  }
  const m = one.moments();
  for (const name of ['mu', 'sigma']) {
    assert.ok(Math.abs(dm[d][name].mean[0] - m[name].mean[0]) <= 1e-12 * Math.abs(m[name].mean[0]) + 1e-13);
    assert.ok(Math.abs(dm[d][name].sd[0] - m[name].sd[0]) <= 1e-10 * Math.abs(m[name].sd[0]));
  }
  one.close();
}
all.close();

const two = new mcmc.AmwgSampler(params, log_post, undefined, Object.assign({ datasets, chains: D * CPD, devices: [0, 0] }, common));
assert.deepStrictEqual(two.info().launch.map((l) => l.chains), [2 * CPD, CPD]);      // datasets 0-1 (a ragged shard) and 2 (an ordinary sampler)
const sharded = run(two);
for (const name of ['mu', 'sigma']) assert.deepStrictEqual(Array.from(sharded[name]), Array.from(got[name]), 'two shards ' + name);
assert.deepStrictEqual(sharded.mu.layout.n_obs, SIZES);
two.close();
console.log('gpu ragged datasets ok');
