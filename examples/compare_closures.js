'use strict';
// compare_closures.js -- two models of ONE dataset compared by PSIS-LOO: a Poisson regression with and without one covariate, both written as ordinary bayes.js
// closures.  options.pointwise: true (beside translate: true) makes the translator write the closure's pointwise terms -- the iterations of its final loop are its
// observations -- so that waic(), loo() and compare_*() work on a closure as they do on a built-in family.   node examples/compare_closures.js
const { mcmc, ld } = require('../bayes.js_amd');
global.ld = ld;

function make_data(n, seed) {      // counts whose rate depends on x1, and only weakly on x2
  let s = seed >>> 0;
  const r = () => { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; };
  const x1 = [], x2 = [], y = [];
  for (let i = 0; i < n; i++) {
    x1.push(2 * r() - 1); x2.push(2 * r() - 1);
    const rate = Math.exp(0.8 + 0.9 * x1[i] + 0.05 * x2[i]);
    let k = 0, p = Math.exp(-rate), c = p;
    const u = r();
    while (u > c && k < 60) { k++; p *= rate / k; c += p; }
    y.push(k);
  }
  return { x1, x2, y };
}

const with_x2 = {
  params: { a: { type: 'real' }, b1: { type: 'real' }, b2: { type: 'real' } },
  log_post: function (state, data) {
    var lp = 0;
    lp += ld.norm(state.a, 0, 5);
    lp += ld.norm(state.b1, 0, 5);
    lp += ld.norm(state.b2, 0, 5);
    for (var i = 0; i < data.y.length; i++) {
      var eta = state.a + state.b1 * data.x1[i] + state.b2 * data.x2[i];
      lp += ld.pois(data.y[i], Math.exp(eta));
    }
    return lp;
  },
};
const without_x2 = {
  params: { a: { type: 'real' }, b1: { type: 'real' } },
  log_post: function (state, data) {
    var lp = 0;
    lp += ld.norm(state.a, 0, 5);
    lp += ld.norm(state.b1, 0, 5);
    for (var i = 0; i < data.y.length; i++) {
      var eta = state.a + state.b1 * data.x1[i];
      lp += ld.pois(data.y[i], Math.exp(eta));
    }
    return lp;
  },
};

function fit(model, data, options) {
  const s = new mcmc.AmwgSampler(model.params, model.log_post, data, Object.assign({ translate: true, pointwise: true, chains: 256, seed: 20261021 }, options || {}));
  s.burn(500);
  s.thin(2);
  s.sample(100);
  const loo = s.loo({ pointwise: true }), waic = s.waic({ pointwise: true });
  if (s.close) s.close();
  return { loo, waic };
}

module.exports = { make_data, with_x2, without_x2, fit };
if (require.main === module) {
  const data = make_data(200, 7);
  const a = fit(with_x2, data), b = fit(without_x2, data);
  const khat = (r) => { const k = r.pointwise.map((t) => t[2]); return { above_0_7: k.filter((v) => v > 0.7).length, above_0_5: k.filter((v) => v > 0.5).length, n: k.length }; };
  console.log('with x2:    elpd_loo %s (se %s), p_loo %s, khat counts %j', a.loo.elpd_loo.toFixed(2), a.loo.se.toFixed(2), a.loo.p_loo.toFixed(2), khat(a.loo));
  console.log('without x2: elpd_loo %s (se %s), p_loo %s, khat counts %j', b.loo.elpd_loo.toFixed(2), b.loo.se.toFixed(2), b.loo.p_loo.toFixed(2), khat(b.loo));
  console.log('compare_loo(with, without): %j', mcmc.compare_loo(a.loo, b.loo));
  console.log('compare_waic(with, without): %j', mcmc.compare_waic(a.waic, b.waic));
}
