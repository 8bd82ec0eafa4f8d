'use strict';
// translate_dataset_tails_cli.js -- test helper: translates the closures of tests/js/dataset_tail_models.js over their datasets with the PRODUCT's translate_datasets and
// writes what translate_datasets_cli.js writes --
//   <out>/<name>.hip, <name>.meta.json, <name>.d<d>.arrays.bin, <name>.own<d>.{hip,meta.json,arrays.bin}
// (the meta also with tail_per_dataset, and `states` / `log_post` under Node as hex bits) -- and beside them
//   <out>/<name>.notail.{hip,meta.json}, <name>.notail.d<d>.arrays.bin   translate_datasets with the caller's no_pois_tail / no_logit_tail
//   <out>/<name>.forced.hip     dataset 0 translated ALONE under the options translate_datasets forced before it knew these tails (no_pois_tail, no_logit_tail,
//                               no_row_plan, no_const_element_fold) and the union of the storage types, is01 and ranges
//   node tests/js/translate_dataset_tails_cli.js <outdir> [name[:n_obs[:n_datasets]] ...]      (a sized variant is written as <name>_<n_obs>, without the .own files)
const fs = require('fs');
const path = require('path');
const { mcmc, ld } = require('../../bayes.js_amd');
const { translate, translate_datasets } = require('../../bayes.js_amd/translate.js');
const dm = require('./dataset_tail_models.js');
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
const NO_TAILS = { no_pois_tail: true, no_logit_tail: true };

for (const spec of (want.length ? want : dm.names)) {
  const [name, nObs, nSets] = spec.split(':');
  const m = dm.build(name, nObs ? Number(nObs) : undefined, nSets ? Number(nSets) : undefined);
  const tag = nObs ? name + '_' + nObs : name;
  const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
  const names = Object.keys(params), plist = [], init = [];
  for (const nm of names) {
    const p = params[nm], len = p.dim.reduce((a, b) => a * b, 1);
    plist.push({ type: p.type, len, top: p.dim[0], multidim: (p.dim.length === 1 && p.dim[0] === 1) ? 0 : 1, lower: p.lower, upper: p.upper });
    const flat = []; (function fl(v) { if (Array.isArray(v)) v.forEach(fl); else flat.push(v); })(p.init);
    flat.forEach((v) => init.push(v));
  }
  // 5 states per dataset with log_post under Node (moderate values: the exponentials stay in range)
  const r = lcg(99), states = [], lps = [];
  m.datasets.slice(0, dm.D).forEach((data) => {
    const ss = [], ll = [];
    for (let k = 0; k < 5; k++) {
      const flat = [], st = {};
      for (const nm of names) {
        const p = params[nm], len = p.dim.reduce((a, b) => a * b, 1), vals = [];
        for (let e = 0; e < len; e++) vals.push(1.5 * r() - 0.5);
        st[nm] = nest(vals, p.dim);
        vals.forEach((v) => flat.push(v));
      }
      ll.push(hex(m.log_post(st, data)));
      ss.push(flat);
    }
    states.push(ss); lps.push(ll);
  });
  const write = (stem, tr) => {
    fs.writeFileSync(path.join(out, stem + '.hip'), tr.source);
    tr.arrays.forEach((arrs, d) => writeArrays(path.join(out, stem + '.d' + d + '.arrays.bin'), arrs));
    fs.writeFileSync(path.join(out, stem + '.meta.json'), JSON.stringify(Object.assign(metaOf(stem, tr), { n_datasets: tr.n_datasets, array_is01: tr.array_is01, array_ranges: tr.array_ranges,
      varying_scalars: tr.varying_scalars, tail_per_dataset: tr.tail_per_dataset, array_len: tr.arrays[0].map((a) => a.length), params: plist, init, states, log_post: lps,
      derived_values: states.map((ss) => ss.map(() => [])) })));
  };
  const tr = translate_datasets(m.log_post, params, m.datasets, {});
  write(tag, tr);
  const off = translate_datasets(m.log_post, params, m.datasets, NO_TAILS);
  write(tag + '.notail', off);
  const byKey = (vals) => { const o = {}; off.array_keys.forEach((k, j) => { o[k] = vals[j]; }); return o; };
  const forced = translate(m.log_post, params, m.datasets[0], Object.assign({ no_row_plan: true, no_const_element_fold: true, array_types: byKey(off.array_types), array_is01: byKey(off.array_is01),
    array_ranges: byKey(off.array_ranges), varying_scalars: new Set(off.varying_scalars) }, NO_TAILS));
  fs.writeFileSync(path.join(out, tag + '.forced.hip'), forced.source);
  if (!nObs) m.datasets.forEach((data, d) => {
    const own = mcmc.translate(m.log_post, params, data, {});
    fs.writeFileSync(path.join(out, tag + '.own' + d + '.hip'), own.source);
    writeArrays(path.join(out, tag + '.own' + d + '.arrays.bin'), own.arrays);
    fs.writeFileSync(path.join(out, tag + '.own' + d + '.meta.json'), JSON.stringify(metaOf(tag, own)));
  });
}
