'use strict';
// pointwise_cli.js -- test helper for options.pointwise.   node tests/js/pointwise_cli.js <out.json> <n> <n_states> [name ...]
// For every accepted closure of tests/js/pointwise_models.js at n observations: the translation with and without { pointwise: true } (the two `source` texts must
// be the same bytes), the pointwise text, the arrays, `n_states` seeded states (flat, in parameter order) and, under V8, term(state, data, i) for each -- the truth the
// device is held to -- after the tie between the two ways of writing the closure: head + the sequential sum of term(i) is log_post(state), bit for bit.
// Also: the refusals of the rejected closures, and the identity of `source` over every closure of tests/js/user_models.js.
// A double travels as the 16 hex digits of its bytes (little-endian): -Infinity and NaN have no JSON.
const fs = require('fs');
const { mcmc, ld } = require('../../bayes.js_amd');
const pm = require('./pointwise_models.js');
const um = require('./user_models.js');
global.ld = ld;
const out = process.argv[2], n = Number(process.argv[3]), nStates = Number(process.argv[4]);
const want = process.argv.slice(5);
const hex = (arr) => Buffer.from(Float64Array.from(arr).buffer).toString('hex');
const same = (a, b) => hex([a]) === hex([b]);

function flatten(params, state) {      // the state object -> components in parameter order (Object.keys(params): mcmc.js:839), row-major
  const flat = [];
  for (const nm of Object.keys(params)) { const v = state[nm]; if (Array.isArray(v)) for (const x of v.flat(Infinity)) flat.push(x); else flat.push(v); }
  return flat;
}

const result = { n, models: {}, rejected: {}, identity: {} };
for (const name of (want.length ? want : pm.names)) {
  if (!pm.CASES[name]) continue;
  const m = pm.build(name, n);
  const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
  const plain = mcmc.translate(m.log_post, params, m.data, {}), tr = mcmc.translate(m.log_post, params, m.data, { pointwise: true });
  const rec = { identical: plain.source === tr.source, why: tr.pointwise_why || null };
  if (tr.pointwise) {
    const r = pm.lcg(4242 + name.length), states = [], terms = [], tie = [];
    for (let s = 0; s < nStates; s++) {
      const st = m.state(r, m.data);
      const row = [];
      let sum = m.head(st, m.data);
      for (let i = 0; i < tr.pointwise.n; i++) { const t = m.term(st, m.data, tr.pointwise.start + i); row.push(t); sum += t; }
      const lp = m.log_post(Object.assign({}, st, Array.isArray(st.theta) ? { theta: st.theta.slice() } : null), m.data);
      tie.push(same(sum, lp) || (Number.isNaN(sum) && Number.isNaN(lp)));
      states.push(hex(flatten(params, st)));
      terms.push(hex(row));
    }
    Object.assign(rec, { source: tr.source, terms_source: tr.pointwise.source, n_obs: tr.pointwise.n, start: tr.pointwise.start, P: tr.P, n_derived: tr.derived.length,
      arrays: tr.arrays.map((a) => hex(Array.from(a))), array_types: tr.array_types, lds_bytes: tr.lds_bytes, lds_bytes_one_lane: tr.lds_bytes_one_lane, parallel: tr.parallel,
      max_threads: tr.max_threads, work_per_eval: tr.work_per_eval, work_one_lane: tr.work_one_lane,
      params: Object.keys(params).map((nm) => ({ name: nm, type: params[nm].type, dim: params[nm].dim, lower: params[nm].lower, upper: params[nm].upper })),
      data: m.data, twin: m.twin || null, bad_obs: m.bad_obs ? m.bad_obs(n) : null, states, terms, tie });
  }
  result.models[name] = rec;
}
if (!want.length) {
  for (const name of pm.rejected) {
    const m = pm.build(name, n);
    const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
    // (a closure the translator refuses altogether -- a derived quantity written in a loop -- has no plan either: the refusal is the translator's own sentence)
    try {
      const plain = mcmc.translate(m.log_post, params, m.data, {}), tr = mcmc.translate(m.log_post, params, m.data, { pointwise: true });
      result.rejected[name] = { identical: plain.source === tr.source, pointwise: tr.pointwise === null ? null : 'a plan', why: tr.pointwise_why || null, expect: m.why };
    } catch (e) { result.rejected[name] = { identical: true, pointwise: null, why: String(e), expect: m.why, thrown: true }; }
  }
  for (const name of um.names) {
    const m = um.build(name);
    const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
    const opts = { helpers: m.helpers, constants: m.constants };
    let a = null, b = null, err = null;
    try { a = mcmc.translate(m.log_post, params, m.data, opts); b = mcmc.translate(m.log_post, params, m.data, Object.assign({ pointwise: true }, opts)); } catch (e) { err = String(e); }
    result.identity[name] = err ? { error: err } : { identical: a.source === b.source, planned: !!b.pointwise, why: b.pointwise_why || null,
      source: b.pointwise ? b.source : undefined, terms_source: b.pointwise ? b.pointwise.source : undefined };      // (the planned texts: compiled by the host test)
  }
}
// `@inf_datasets` among the names: the minus_inf closure over three datasets under ONE source (translate_datasets) -- the middle one holds the -Infinity observation,
// the outer two a sound count in its place
if (want.indexOf('@inf_datasets') >= 0) {
  const { translate_datasets } = require('../../bayes.js_amd/translate.js');
  const bad = pm.build('minus_inf', n), at = bad.bad_obs(n);
  const sound = (seed) => { const d = pm.build('minus_inf', n, seed).data; d.y[at] = 2; return d; };
  const sets = [sound(7), bad.data, sound(9)];
  const params = mcmc.complete_params(bad.params, mcmc.param_init_fixed);
  const tr = translate_datasets(bad.log_post, params, sets, { pointwise: true });
  result.inf_datasets = { source: tr.source, terms_source: tr.pointwise.source, n_obs: tr.pointwise.n, P: tr.P, n_derived: tr.derived.length, bad_obs: at,
    arrays: tr.arrays.map((row) => row.map((a) => hex(Array.from(a)))), array_types: tr.array_types, lds_bytes: tr.lds_bytes, lds_bytes_one_lane: tr.lds_bytes_one_lane,
    parallel: tr.parallel, max_threads: tr.max_threads, work_per_eval: tr.work_per_eval, work_one_lane: tr.work_one_lane };
}
fs.writeFileSync(out, JSON.stringify(result));
