'use strict';
// The README model (README.md:18-43) on 64 datasets in one sampler (options.datasets): per dataset the 95 % highest-density interval of mu and sigma next to
// the equal-tailed interval of dataset_quantiles([0.025, 0.975]).  For the symmetric posterior of mu the two nearly agree; sigma's posterior is skewed to the
// right, so its highest-density interval sits lower and is shorter -- it is the shortest interval holding 95 % of the draws.  Both are formed on the device:
//   node examples/hpd_datasets.js
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

// 64 small samples of 12 heights: few observations, so sigma's posterior has a long right tail
var datasets = [];
for (var d = 0; d < 64; d++) {
  var x = [];
  for (var i = 0; i < 12; i++) x.push(mcmc.rnorm(160 + 0.25 * d, 7));
  datasets.push(x);
}

var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, chains: 64 * 256, seed: 1 });
sampler.burn(1000);
sampler.sample_on_device(400);
var hdi = sampler.dataset_hpd([0.95]), eti = sampler.dataset_quantiles([0.025, 0.975]);
var f = function (v) { return v.toFixed(2); };
[0, 1, 32, 63].forEach(function (d) {
  ['mu', 'sigma'].forEach(function (name) {
    var h = hdi[d][name][0][0], q = eti[d][name][0];
    console.log('dataset %d %s: 95%% HDI [%s, %s] (width %s)   equal-tailed [%s, %s] (width %s)', d, name, f(h[0]), f(h[1]), f(h[1] - h[0]), f(q[0]), f(q[1]), f(q[1] - q[0]));
  });
});
sampler.close();
