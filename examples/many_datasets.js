'use strict';
// The README model (README.md:18-43) on 256 datasets at once: one posterior per dataset, 256 chains each, ONE sampler and one launch per call
// (options.datasets) -- what a loop over 256 samplers would otherwise do, a workgroup per launch:
//   node examples/many_datasets.js
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

// 256 synthetic samples of 1000 heights; the true mean differs per dataset
var datasets = [];
for (var d = 0; d < 256; d++) {
  var x = [];
  for (var i = 0; i < 1000; i++) x.push(mcmc.rnorm(160 + 0.1 * d, 7));
  datasets.push(x);
}

// the data argument is null: options.datasets takes its place; options.chains is the total
var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, chains: 256 * 256, seed: 1 });
sampler.burn(1000);
sampler.sample_on_device(200);
var moments = sampler.dataset_moments(), conv = sampler.dataset_convergence();
var quant = sampler.dataset_quantiles([0.025, 0.5, 0.975]);      // a 95 % credible interval and the median per dataset, selected on the device
[0, 1, 128, 255].forEach(function (d) {
  var q = quant[d].mu[0];
  console.log('dataset %d (true mean %s): mean(mu) = %s  median(mu) = %s  95%% interval [%s, %s]  mean(sigma) = %s  Rhat(mu) = %s', d, (160 + 0.1 * d).toFixed(1),
    moments[d].mu.mean[0].toFixed(2), q[1].toFixed(2), q[0].toFixed(2), q[2].toFixed(2), moments[d].sigma.mean[0].toFixed(2), conv[d].mu.rhat[0].toFixed(4));
});
console.log('kernel:', sampler.info().launch[0].kernel, ' datasets per launch:', sampler.info().launch[0].datasets);
sampler.close();
