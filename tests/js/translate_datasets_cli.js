'use strict';
// translate_datasets_cli.js -- test helper: translates the closures of tests/js/dataset_models.js over their D datasets with the PRODUCT's translate_datasets and writes
//   <out>/<name>.hip            the one source
//   <out>/<name>.meta.json      translate_cli.js's fields, plus n_datasets, array_is01, array_ranges, varying_scalars, the params as the C ABI wants them,
//                               `states` (5 per dataset, drawn from a fixed seed) and `log_post` = log_post(states[d][k], datasets[d]) under Node with ld.js, as hex bits,
//                               and `derived_values` likewise
//   <out>/<name>.d<d>.arrays.bin   dataset d's arrays (u32 count, then per array u64 len + f64 data)
//   <out>/<name>.own<d>.*       the DEFAULT translation of dataset d alone (translate()), for the independent one-lane comparison
//   <out>/refusals.json         {name: message} for the closures translate_datasets must refuse
//   node tests/js/translate_datasets_cli.js <outdir> [name[:n_obs[:n_datasets]] ...]      (a sized variant is written as <name>_<n_obs>, without the .own files)
const fs = require('fs');
const path = require('path');
const { mcmc, ld } = require('../../bayes.js_amd');
const { translate_datasets } = require('../../bayes.js_amd/translate.js');
const dm = require('./dataset_models.js');
global.ld = ld;
const out = process.argv[2];
const want = process.argv.slice(3);

function writeArrays(file, arrays) {
  let bytes = 4;
  for (const a of arrays) bytes += 8 + a.length * 8;
  const buf = Buffer.alloc(bytes);
  let o = 0;
  buf.writeUInt32LE(arrays.length, o); o += 4;
  for (const a of arrays) {
    buf.writeBigUInt64LE(BigInt(a.length), o); o += 8;
    for (let i = 0; i < a.length; i++) { buf.writeDoubleLE(a[i], o); o += 8; }
  }
  fs.writeFileSync(file, buf);
}
const metaOf = (name, tr) => ({ name, P: tr.P, derived: tr.derived, lds_bytes: tr.lds_bytes, lds_bytes_one_lane: tr.lds_bytes_one_lane, parallel: tr.parallel, max_threads: tr.max_threads,
  work_per_eval: tr.work_per_eval, work_one_lane: tr.work_one_lane, rows_n_obs: tr.rows_n_obs, rows_groups: tr.rows_groups, rows_sweep: tr.rows_sweep, cert_tail_n: tr.cert_tail_n,
  rows_cert: tr.rows_cert, pois_tail_n: tr.pois_tail_n, logit_tail_n: tr.logit_tail_n, array_keys: tr.array_keys, array_types: tr.array_types });
const hex = (v) => { const b = Buffer.alloc(8); b.writeDoubleBE(v, 0); return b.toString('hex'); };
function lcg(seed) { let s = seed >>> 0; return () => { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; }; }
function nest(flat, dim) { return dim.length === 1 && dim[0] === 1 ? flat[0] : flat.slice(); }

for (const spec of (want.length ? want : dm.names)) {
  const [name, nObs, nSets] = spec.split(':');
  const m = dm.build(name, nObs ? Number(nObs) : undefined, nSets ? Number(nSets) : undefined);
  const tag = nObs ? name + '_' + nObs : name;
  const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
  const tr = translate_datasets(m.log_post, params, m.datasets, {});
  fs.writeFileSync(path.join(out, tag + '.hip'), tr.source);
  tr.arrays.forEach((arrs, d) => writeArrays(path.join(out, tag + '.d' + d + '.arrays.bin'), arrs));
  // parameters in Object.keys order, as the C ABI takes them; states for the host comparison
  const names = Object.keys(params), plist = [], init = [];
  for (const nm of names) {
    const p = params[nm], len = p.dim.reduce((a, b) => a * b, 1);
    plist.push({ type: p.type, len, top: p.dim[0], multidim: (p.dim.length === 1 && p.dim[0] === 1) ? 0 : 1, lower: p.lower, upper: p.upper });
    const flat = []; (function fl(v) { if (Array.isArray(v)) v.forEach(fl); else flat.push(v); })(p.init);
    flat.forEach((v) => init.push(v));
  }
  const r = lcg(99), states = [], lps = [], dvs = [];
  m.datasets.forEach((data) => {
    const ss = [], ll = [], dd = [];
    for (let k = 0; k < 5; k++) {
      const flat = [], st = {};
      for (const nm of names) {
        const p = params[nm], len = p.dim.reduce((a, b) => a * b, 1), vals = [];
        for (let e = 0; e < len; e++) vals.push(Number.isFinite(p.lower) && p.lower >= 0 ? 0.5 + 3 * r() : 4 * r() - 1.5);
        st[nm] = nest(vals, p.dim);
        vals.forEach((v) => flat.push(v));
      }
      ll.push(hex(m.log_post(st, data)));
      dd.push(tr.derived.map((q) => hex(st[q])));
      ss.push(flat);
    }
    states.push(ss); lps.push(ll); dvs.push(dd);
  });
  fs.writeFileSync(path.join(out, tag + '.meta.json'), JSON.stringify(Object.assign(metaOf(tag, tr), { n_datasets: tr.n_datasets, array_is01: tr.array_is01, array_ranges: tr.array_ranges,
    varying_scalars: tr.varying_scalars, array_len: tr.arrays[0].map((a) => a.length), params: plist, init, states, log_post: lps, derived_values: dvs })));
  // every dataset's own default translation
  if (!nObs) m.datasets.forEach((data, d) => {
    const own = mcmc.translate(m.log_post, params, data, {});
    fs.writeFileSync(path.join(out, tag + '.own' + d + '.hip'), own.source);
    writeArrays(path.join(out, tag + '.own' + d + '.arrays.bin'), own.arrays);
    fs.writeFileSync(path.join(out, tag + '.own' + d + '.meta.json'), JSON.stringify(metaOf(tag, own)));
  });
}
if (!want.length) {
  const refusals = {};
  for (const name of dm.refused) {
    const m = dm.build(name);
    try { translate_datasets(m.log_post, mcmc.complete_params(m.params, mcmc.param_init_fixed), m.datasets, {}); refusals[name] = null; }
    catch (e) { refusals[name] = String(e && e.message ? e.message : e); }
  }
  fs.writeFileSync(path.join(out, 'refusals.json'), JSON.stringify(refusals));
}
