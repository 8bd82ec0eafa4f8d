'use strict';
// translate_logit_cli.js -- test helper: translates closures of tests/js/logit_models.js with the PRODUCT's translator, in the file layout of translate_cli.js
// (<label>.hip, <label>.arrays.bin, <label>.meta.json -- the meta with logit_tail_n).
//   node tests/js/translate_logit_cli.js <outdir> <name>[@n[@ymode]] ...      label = the argument with '@' replaced by '_'
//   $AMWG_TRANSLATE_OPTS: extra translator options as JSON (e.g. {"no_logit_tail":true})
const fs = require('fs');
const path = require('path');
const { mcmc, ld } = require('../../bayes.js_amd');
const lm = require('./logit_models.js');
global.ld = ld;
const out = process.argv[2];
for (const arg of process.argv.slice(3)) {
  const [name, n, ymode] = arg.split('@');
  const label = arg.replace(/@/g, '_');
  const m = lm.build(name, n ? Number(n) : undefined, ymode);
  const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
  const tr = mcmc.translate(m.log_post, params, m.data, JSON.parse(process.env.AMWG_TRANSLATE_OPTS || '{}'));
  fs.writeFileSync(path.join(out, label + '.hip'), tr.source);
  let bytes = 4;
  for (const a of tr.arrays) bytes += 8 + a.length * 8;
  const buf = Buffer.alloc(bytes);
  let o = 0;
  buf.writeUInt32LE(tr.arrays.length, o); o += 4;
  for (const a of tr.arrays) {
    buf.writeBigUInt64LE(BigInt(a.length), o); o += 8;
    for (let i = 0; i < a.length; i++) { buf.writeDoubleLE(a[i], o); o += 8; }
  }
  fs.writeFileSync(path.join(out, label + '.arrays.bin'), buf);
  fs.writeFileSync(path.join(out, label + '.meta.json'), JSON.stringify({ name: label, P: tr.P, derived: tr.derived, lds_bytes: tr.lds_bytes, lds_bytes_one_lane: tr.lds_bytes_one_lane,
    parallel: tr.parallel, max_threads: tr.max_threads, work_per_eval: tr.work_per_eval, work_one_lane: tr.work_one_lane, rows_n_obs: tr.rows_n_obs, rows_groups: tr.rows_groups, rows_sweep: tr.rows_sweep,
    cert_tail_n: tr.cert_tail_n, rows_cert: tr.rows_cert, pois_tail_n: tr.pois_tail_n, logit_tail_n: tr.logit_tail_n, array_keys: tr.array_keys, array_types: tr.array_types, array_len: tr.arrays.map((a) => a.length) }));
}
