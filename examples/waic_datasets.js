'use strict';
// The README model (README.md:18-43) on 64 small datasets in one sampler (options.datasets): per dataset WAIC -- the expected log pointwise predictive density
// elpd_waic with its standard error, and p_waic, the effective number of parameters (near 2 here: mu and sigma) -- formed on the device from the stored draws.
// high_variance counts the observations whose p_i exceeds 0.4, where WAIC is unreliable.  (mcmc.compare_waic(a, b) compares two fits of the same observations.)
//   node examples/waic_datasets.js
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

// 64 samples of 50 heights
var datasets = [];
for (var d = 0; d < 64; d++) {
  var x = [];
  for (var i = 0; i < 50; i++) x.push(mcmc.rnorm(160 + 0.25 * d, 7));
  datasets.push(x);
}

var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, chains: 64 * 256, seed: 1 });
sampler.burn(1000);
sampler.sample_on_device(400);
var w = sampler.dataset_waic({ pointwise: true });
var f = function (v) { return v.toFixed(2); };
w.forEach(function (r, d) {
  console.log('dataset %d: elpd_waic %s +- %s   p_waic %s   waic %s   high-variance observations %d', d, f(r.elpd_waic), f(r.se), f(r.p_waic), f(r.waic), r.high_variance);
});
sampler.close();
