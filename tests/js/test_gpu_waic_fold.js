'use strict';
// summarize(n, {waic: true}) of the JavaScript front end on the GPU: the README Normal closure on one dataset.  The folded waic() against the stored run of the same
// seed -- the same draws, so the pairs agree far inside the header's bounds --, dataset_waic() as its one entry, compare_waic() between two folded fits, waic_info(),
// and the refusals: loo() after any summarising call, waic() after one without the option.
const assert = require('assert');
const { mcmc, ld } = require('../../bayes.js_amd');
global.ld = ld;

var params = {
  mu: {type: "real"},
  sigma: {type: "real", lower: 0} };
var log_post = function(state, data) {
  var log_post = 0;
  log_post += ld.norm(state.mu, 0, 100);
  log_post += ld.unif(state.sigma, 0, 100);
  for(var i = 0; i < data.length; i++) {
    log_post += ld.norm(data[i], state.mu, state.sigma);
  }
  return log_post;
};

const N = mcmc.native(), SEED = 20261126, KEPT = 60, WINDOW = 7;
const x = [];
for (let i = 0; i < 75; i++) { let s = 0; for (let k = 0; k < 12; k++) s += N.uniform(951, 1, i * 12 + k); x.push(175 + 7 * (s - 6)); }
const make = (seed) => { const s = new mcmc.AmwgSampler(params, log_post, x, { seed, chains: 64, lanes_per_chain: 1, block_threads: 64 }); s.burn(1000); return s; };
const message = (e) => String(e && e.message ? e.message : e);

const stored = make(SEED), folded = make(SEED), other = make(SEED + 1);
stored.sample_on_device(KEPT);
const ws = stored.waic({ pointwise: true });
assert.strictEqual(folded.waic_info().armed, false);
assert.strictEqual(folded.summarize(KEPT, { waic: true, window_rows: WINDOW }), KEPT);
const info = folded.waic_info();
assert.ok(info.armed && info.bytes === 32 * x.length, JSON.stringify(info));      // 7 x 64 draws a window: one split
const wf = folded.waic({ pointwise: true });
assert.deepStrictEqual(Object.keys(wf), Object.keys(ws));
assert.strictEqual(wf.pointwise.length, x.length);
let worst = 0;
for (let i = 0; i < x.length; i++) for (let k = 0; k < 2; k++) worst = Math.max(worst, Math.abs(wf.pointwise[i][k] - ws.pointwise[i][k]));
console.log('folded against stored, ' + KEPT * 64 + ' draws in windows of ' + WINDOW + ' rows: largest difference of a pair ' + worst.toExponential(2) + '; elpd ' + wf.elpd_waic.toFixed(3) + ' vs ' + ws.elpd_waic.toFixed(3));
assert.ok(worst < 1e-9 && Math.abs(wf.elpd_waic - ws.elpd_waic) < 1e-7);
assert.deepStrictEqual(folded.dataset_waic({ pointwise: true }), [wf]);
assert.ok(!('pointwise' in folded.waic()));

other.summarize(KEPT, { waic: true });
const cmp = mcmc.compare_waic(wf, other.waic({ pointwise: true }));
assert.ok(Math.abs(cmp.elpd_diff) < 1 && cmp.se_diff >= 0, JSON.stringify(cmp));      // two runs of one model: the same fit
assert.deepStrictEqual(mcmc.compare_waic(wf, wf), { elpd_diff: 0, se_diff: 0 });

assert.throws(() => folded.loo(), (e) => /amwg_last_sample_dataset_loo/.test(message(e)) && /amwg_sample_summarize/.test(message(e)));
folded.summarize(KEPT);      // the option holds for one call
assert.strictEqual(folded.waic_info().armed, false);
assert.throws(() => folded.waic(), (e) => /amwg_last_sample_dataset_waic/.test(message(e)) && /amwg_sample_summarize/.test(message(e)) && /amwg_set_waic/.test(message(e)));
for (const s of [stored, folded, other]) s.close();
console.log('gpu waic fold ok');
