'use strict';
// translate_truncated_cli.js -- test helper: translates a closure of tests/js/user_models.js whose data IS one array (the README shape: bench_normal) with the
// array cut to its first n values, and writes the same three files as translate_cli.js under <outname>.
//   node tests/js/translate_truncated_cli.js <outdir> <name> <n> <outname>
const fs = require('fs');
const path = require('path');
const { mcmc, ld } = require('../../bayes.js_amd');
const um = require('./user_models.js');
global.ld = ld;
const [out, name, nArg, outname] = process.argv.slice(2);
const m = um.build(name);
const data = Array.from(m.data).slice(0, Number(nArg));
if (data.length !== Number(nArg)) throw new Error(name + ' has fewer than ' + nArg + ' observations');
const params = mcmc.complete_params(m.params, mcmc.param_init_fixed);
const tr = mcmc.translate(m.log_post, params, data, { helpers: m.helpers, constants: m.constants });
fs.writeFileSync(path.join(out, outname + '.hip'), tr.source);
let bytes = 4;
for (const a of tr.arrays) bytes += 8 + a.length * 8;
const buf = Buffer.alloc(bytes);
let o = 0;
buf.writeUInt32LE(tr.arrays.length, o); o += 4;
for (const a of tr.arrays) {
  buf.writeBigUInt64LE(BigInt(a.length), o); o += 8;
  for (let i = 0; i < a.length; i++) { buf.writeDoubleLE(a[i], o); o += 8; }
}
fs.writeFileSync(path.join(out, outname + '.arrays.bin'), buf);
fs.writeFileSync(path.join(out, outname + '.meta.json'), JSON.stringify({ name: outname, P: tr.P, derived: tr.derived, lds_bytes: tr.lds_bytes, lds_bytes_one_lane: tr.lds_bytes_one_lane,
  parallel: tr.parallel, max_threads: tr.max_threads, work_per_eval: tr.work_per_eval, work_one_lane: tr.work_one_lane, rows_n_obs: tr.rows_n_obs, rows_groups: tr.rows_groups, rows_sweep: tr.rows_sweep, cert_tail_n: tr.cert_tail_n, rows_cert: tr.rows_cert, pois_tail_n: tr.pois_tail_n, array_keys: tr.array_keys, array_types: tr.array_types, array_len: tr.arrays.map((a) => a.length) }));
