'use strict';
// time_pointwise_translate.js -- helper of tools/time_pointwise.py: one closure of tests/js/pointwise_models.js translated over D datasets of n observations with
// { pointwise: true } (translate_datasets: one source, one pointwise text), written as JSON; a double travels as the hex of its bytes.
//   node tools/time_pointwise_translate.js <out.json> <name> <D> <n>
const fs = require('fs');
const { mcmc, ld } = require('../bayes.js_amd');
const pm = require('../tests/js/pointwise_models.js');
const translator = require('../bayes.js_amd/translate.js');
global.ld = ld;
const [out, name, D, n] = [process.argv[2], process.argv[3], Number(process.argv[4]), Number(process.argv[5])];
const hex = (arr) => Buffer.from(Float64Array.from(arr).buffer).toString('hex');
const sets = [];
for (let d = 0; d < D; d++) sets.push(pm.build(name, n, 500 + d));
const params = mcmc.complete_params(sets[0].params, mcmc.param_init_fixed);
const tr = D > 1 ? translator.translate_datasets(sets[0].log_post, params, sets.map((s) => s.data), { pointwise: true })
                 : mcmc.translate(sets[0].log_post, params, sets[0].data, { pointwise: true });
if (!tr.pointwise) throw new Error(tr.pointwise_why);
const arrays = D > 1 ? tr.arrays : [tr.arrays];
fs.writeFileSync(out, JSON.stringify({ name, D, n, source: tr.source, terms_source: tr.pointwise.source, n_obs: tr.pointwise.n, P: tr.P, n_derived: tr.derived.length,
  array_types: tr.array_types, lds_bytes: tr.lds_bytes, lds_bytes_one_lane: tr.lds_bytes_one_lane, parallel: tr.parallel, max_threads: tr.max_threads,
  work_per_eval: tr.work_per_eval, work_one_lane: tr.work_one_lane, arrays: arrays.map((row) => row.map((a) => hex(Array.from(a)))),
  data: sets.map((s) => (Array.isArray(s.data) ? hex(s.data) : null)) }));
