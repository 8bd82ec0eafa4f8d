'use strict';
// options.datasets with options.translate: true on the GPU for a closure that ends in a logistic-regression loop (dst_logit of tests/js/dataset_tail_models.js): three
// datasets x 8 chains in ONE sampler at 16 lanes per chain run the certified dataset twin, and each dataset's slice of sample() deep-equals an ordinary sampler on
// datasets[d] -- ITS OWN default translation, the existing amwg_user_step_cert -- with chain_offset d * 8 (both are the reference's chain).
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;
const dm = require('./dataset_tail_models.js');

const m = dm.build('dst_logit'), D = 3, CPD = 8, SEED = 20261018, KEPT = 14, LEN = 4;
const common = { seed: SEED, lanes_per_chain: 16, block_threads: 64 };
function run(s) { s.burn(120); s.thin(3); return s.sample(40); }

const all = new mcmc.AmwgSampler(m.params, m.log_post, undefined, Object.assign({ datasets: m.datasets, translate: true, chains: D * CPD }, common));
const launch = all.info().launch[0];
assert.ok(launch.kernel === 'amwg_user_step_cert_ds' && launch.datasets === D && launch.summation_order === 1, JSON.stringify(launch));
const got = run(all);
assert.deepStrictEqual(got.b.layout, { kept: KEPT, len: LEN, chains: D * CPD, dim: [LEN], datasets: D, chains_per_dataset: CPD });
const slice = (arr, d) => { const o = []; for (let t = 0; t < KEPT; t++) for (let e = 0; e < LEN; e++) o.push(Array.from(arr.subarray((t * LEN + e) * D * CPD + d * CPD, (t * LEN + e) * D * CPD + (d + 1) * CPD))); return o; };
const rows = (arr, C) => { const o = []; for (let r = 0; r < KEPT * LEN; r++) o.push(Array.from(arr.subarray(r * C, (r + 1) * C))); return o; };
const moments = all.dataset_moments();
assert.strictEqual(moments.length, D);
for (let d = 0; d < D; d++) {
  const one = new mcmc.AmwgSampler(m.params, m.log_post, m.datasets[d], Object.assign({ chains: CPD, chain_offset: d * CPD }, common));
  assert.strictEqual(one.info().launch[0].kernel, 'amwg_user_step_cert');
  const want = run(one);
  assert.deepStrictEqual(slice(got.b, d), rows(want.b, CPD), 'dataset ' + d);
  one.close();
  assert.ok(moments[d].b.mean.every(Number.isFinite));
}
all.close();
console.log('gpu user dataset tails ok');
