'use strict';
// options.pointwise of the JavaScript front end on the GPU: the two Poisson regressions of examples/compare_closures.js (with and without one covariate) fitted to
// ONE dataset as translated closures; loo() and waic() answer with an entry per observation of the final loop; compare_loo / compare_waic of the two models give a
// finite difference whose sign agrees with the totals; a model compared with itself gives zeros; a closure sampler made WITHOUT the flag keeps the library's
// refusal, word for word.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;
const ex = require('../../examples/compare_closures.js');

const data = ex.make_data(65, 11), common = { chains: 64, lanes_per_chain: 1 };
function fit(model, options) {
  const s = new mcmc.AmwgSampler(model.params, model.log_post, data, Object.assign({ translate: true, seed: 20261021 }, common, options));
  s.burn(200);
  s.sample(30);
  return s;
}
const a = fit(ex.with_x2, { pointwise: true }), b = fit(ex.without_x2, { pointwise: true });
const la = a.loo({ pointwise: true }), lb = b.loo({ pointwise: true }), wa = a.waic({ pointwise: true }), wb = b.waic({ pointwise: true });
for (const r of [la, lb]) {
  assert.strictEqual(r.pointwise.length, 65);
  assert(Number.isFinite(r.elpd_loo) && Number.isFinite(r.se) && r.pointwise.every((t) => t.length === 3 && Number.isFinite(t[0]) && Number.isFinite(t[1])));
}
for (const r of [wa, wb]) assert(r.pointwise.length === 65 && Number.isFinite(r.elpd_waic) && r.pointwise.every((t) => t.length === 2 && Number.isFinite(t[0]) && t[1] >= 0));
for (let i = 0; i < 65; i++) assert(Object.is(la.pointwise[i][1], wa.pointwise[i][0]));      // lppd_i is WAIC's
const cl = mcmc.compare_loo(la, lb), cw = mcmc.compare_waic(wa, wb);
assert(Number.isFinite(cl.elpd_diff) && Number.isFinite(cl.se_diff) && cl.se_diff >= 0);
assert(Math.abs(cl.elpd_diff - (la.elpd_loo - lb.elpd_loo)) <= 1e-9 * (1 + Math.abs(la.elpd_loo)));
assert(Math.abs(cw.elpd_diff - (wa.elpd_waic - wb.elpd_waic)) <= 1e-9 * (1 + Math.abs(wa.elpd_waic)));
const self = mcmc.compare_loo(la, la), selfw = mcmc.compare_waic(wa, wa);
assert(self.elpd_diff === 0 && self.se_diff === 0 && selfw.elpd_diff === 0 && selfw.se_diff === 0);
const again = a.loo({ pointwise: true });
assert(again.pointwise.every((t, i) => [0, 1, 2].every((k) => Object.is(t[k], la.pointwise[i][k]))));      // repeat calls: the same numbers
assert.strictEqual(a.dataset_loo().length, 1);
console.log('compare_loo(with x2, without x2) = %j; khat > 0.7: %d and %d of 65', cl, la.high_k, lb.high_k);

const plain = fit(ex.without_x2, {});
for (const call of ['waic', 'loo']) {
  let msg = '';
  try { plain[call](); } catch (e) { msg = String(e && e.message ? e.message : e); }
  assert(msg.indexOf('the pointwise terms of a closure are not known to the library; built-in families only') >= 0, msg);
}
console.log('ok');
