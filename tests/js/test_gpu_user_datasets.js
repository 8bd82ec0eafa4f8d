'use strict';
// options.datasets with options.translate: true on the GPU: the closure ds_mixed of tests/js/dataset_models.js (no built-in family; storage types, label ranges and a
// scalar that differ between the datasets; a derived quantity) on three datasets x 64 chains in ONE sampler, one lane per chain.  Each dataset's slice of sample()
// deep-equals an ordinary sampler on datasets[d] -- ITS OWN default translation -- with chain_offset d * 64 (one lane per chain is the reference's order in both);
// dataset_quantiles matches a sort; the pooled summaries throw; dealing the datasets to two shards (devices: [0, 0]: datasets 0-1 and 2) returns the same draws.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;
const dm = require('./dataset_models.js');

const m = dm.build('ds_mixed'), D = 3, CPD = 64, SEED = 20261018, KEPT = 14;
const common = { seed: SEED, lanes_per_chain: 1, block_threads: 64 };
function run(s) { s.burn(120); s.thin(3); return s.sample(40); }
const NAMES = ['theta', 'b', 'spread'];

const all = new mcmc.AmwgSampler(m.params, m.log_post, null, Object.assign({ datasets: m.datasets, translate: true, chains: D * CPD }, common));
const got = run(all);
assert.deepStrictEqual(got.b.layout, { kept: KEPT, len: 1, chains: D * CPD, dim: [1], datasets: D, chains_per_dataset: CPD });
assert.deepStrictEqual(got.theta.layout.dim, [3]);
const launch = all.info().launch[0];
assert.ok(launch.kernel === 'amwg_user_step_ds' && launch.datasets === D, JSON.stringify(launch));
assert.strictEqual(all.data, m.datasets[0]);      // what the host-side log_post() evaluates against: dataset 0
assert.deepStrictEqual(all.derived, ['spread']);
// [kept][len][chains] -> dataset d's [kept][len][cpd]
const slice = (arr, len, d) => { const o = []; for (let t = 0; t < KEPT; t++) for (let e = 0; e < len; e++) o.push(Array.from(arr.subarray((t * len + e) * D * CPD + d * CPD, (t * len + e) * D * CPD + (d + 1) * CPD))); return o; };
const rows = (arr, len, C) => { const o = []; for (let r = 0; r < KEPT * len; r++) o.push(Array.from(arr.subarray(r * C, (r + 1) * C))); return o; };
const probs = [0.025, 0.5, 0.975];
const moments = all.dataset_moments(), conv = all.dataset_convergence(), quant = all.dataset_quantiles(probs);
assert.strictEqual(moments.length, D);
assert.strictEqual(conv.length, D);
assert.strictEqual(quant.length, D);
for (const f of [() => all.moments(), () => all.convergence(), () => all.quantiles([0.5])])
  assert.throws(f, (e) => /amwg_last_sample_dataset_moments/.test(String(e && e.message ? e.message : e)));
const type7 = (sorted, q) => { const h = (sorted.length - 1) * q, lo = Math.floor(h), hi = Math.min(lo + 1, sorted.length - 1); return sorted[lo] + (h - lo) * (sorted[hi] - sorted[lo]); };
for (let d = 0; d < D; d++) {
  const one = new mcmc.AmwgSampler(m.params, m.log_post, m.datasets[d], Object.assign({ chains: CPD, chain_offset: d * CPD }, common));
  const want = run(one);
  for (const name of NAMES) {
    const len = name === 'theta' ? 3 : 1;
    assert.deepStrictEqual(slice(got[name], len, d), rows(want[name], len, CPD), 'dataset ' + d + ' ' + name);
  }
  one.close();
  // quantiles: type 7 over a sort of the dataset's slice, bit for bit (theta[1] and the derived quantity)
  for (const [name, len, e] of [['theta', 3, 1], ['spread', 1, 0]]) {
    const vals = [];
    for (let t = 0; t < KEPT; t++) for (let c = 0; c < CPD; c++) vals.push(got[name][(t * len + e) * D * CPD + d * CPD + c]);
    const sorted = Float64Array.from(vals).sort();
    assert.deepStrictEqual(quant[d][name][e], probs.map((q) => type7(sorted, q)), 'quantiles of dataset ' + d + ' ' + name);
  }
  assert.strictEqual(moments[d].theta.mean.length, 3);
  assert.ok(Number.isFinite(moments[d].spread.mean[0]) && (d === 2 || Number.isFinite(conv[d].b.rhat[0])));      // (dataset 2: log_post is -Infinity, its chains never move)
}
all.close();

const two = new mcmc.AmwgSampler(m.params, m.log_post, undefined, Object.assign({ datasets: m.datasets, translate: true, chains: D * CPD, devices: [0, 0] }, common));
assert.deepStrictEqual(two.info().launch.map((l) => [l.chains, l.kernel]), [[2 * CPD, 'amwg_user_step_ds'], [CPD, 'amwg_user_step']]);      // datasets 0-1, and 2 alone
const sharded = run(two);
for (const name of NAMES) assert.deepStrictEqual(Array.from(sharded[name]), Array.from(got[name]), 'two shards ' + name);
assert.strictEqual(two.dataset_moments().length, D);
assert.throws(() => two.moments());
two.close();
console.log('gpu user datasets ok');
