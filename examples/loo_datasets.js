'use strict';
// The README model (README.md:18-43) on 64 small datasets in one sampler (options.datasets), each with ONE PLANTED OUTLIER: per dataset elpd_waic beside elpd_loo,
// both formed on the device from the stored draws.  WAIC warns about the outlier (its p_i exceeds 0.4: high_variance); PSIS-LOO is what to use then: it leaves each
// observation out by importance sampling, smooths the largest weights with a generalised Pareto fit, and reports the fit's shape khat per observation -- above 0.7 the
// estimate for that observation is unreliable too (high_k).  (mcmc.compare_loo(a, b) compares two fits of the same observations.)
//   node examples/loo_datasets.js
const { mcmc, ld } = require('../bayes.js_amd');
global.ld = ld;

var params = {
  mu: {type: "real"},
  sigma: {type: "real", lower: 0}};

var log_post = function(state, data) {
  var log_post = 0;
  // Priors
  log_post += ld.norm(state.mu, 0, 100);
  log_post += ld.unif(state.sigma, 0, 100);
  // Likelihood
  for(var i = 0; i < data.length; i++) {
    log_post += ld.norm(data[i], state.mu, state.sigma);
  }
  return log_post;
};

// 64 samples of 50 heights; the last height of each is 35 cm off
var OUTLIER = 49;
var datasets = [];
for (var d = 0; d < 64; d++) {
  var x = [];
  for (var i = 0; i < 50; i++) x.push(mcmc.rnorm(160 + 0.25 * d, 7));
  x[OUTLIER] += 35;
  datasets.push(x);
}

var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, chains: 64 * 256, seed: 1 });
sampler.burn(1000);
sampler.sample_on_device(400);
var w = sampler.dataset_waic({ pointwise: true }), l = sampler.dataset_loo({ pointwise: true });
var f = function (v) { return v.toFixed(2); };
l.forEach(function (r, d) {
  var o = r.pointwise[OUTLIER];
  console.log('dataset %d: elpd_waic %s   elpd_loo %s +- %s   p_loo %s   the outlier: p_i %s, khat %s, elpd_loo_i %s   high_variance %d high_k %d', d, f(w[d].elpd_waic), f(r.elpd_loo),
              f(r.se), f(r.p_loo), f(w[d].pointwise[OUTLIER][1]), f(o[2]), f(o[0]), w[d].high_variance, r.high_k);
});
sampler.close();
