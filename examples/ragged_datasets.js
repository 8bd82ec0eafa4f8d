'use strict';
// The README model (README.md:18-43) on 64 segments of UNEQUAL size at once -- one A/B test per segment, and segments are never of one size: one
// posterior per segment, 256 chains each, ONE sampler and one launch per call.  options.datasets takes the segments as they are; nothing says "ragged":
//   node examples/ragged_datasets.js
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

// 64 synthetic segments of 20 to ~5000 heights (sizes spread log-uniformly); the true mean differs per segment.  Largest first: the workgroups of the
// big segments are then dispatched first and the small ones fill the tail (DESIGN.md section 6)
var datasets = [];
for (var d = 0; d < 64; d++) {
  var n = Math.round(20 * Math.pow(250, (63 - d) / 63)), x = [];
  for (var i = 0; i < n; i++) x.push(mcmc.rnorm(160 + 0.1 * d, 7));
  datasets.push(x);
}

// the data argument is null: options.datasets takes its place; options.chains is the total
var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, chains: 64 * 256, seed: 1 });
sampler.burn(1000);
var draws = sampler.sample(200);
var sizes = draws.mu.layout.n_obs;      // the segments' sizes, beside datasets / chains_per_dataset
var moments = sampler.dataset_moments();
var quant = sampler.dataset_quantiles([0.025, 0.975]);      // a 95 % credible interval per segment, selected on the device
[0, 1, 32, 63].forEach(function (d) {
  var q = quant[d].mu[0];
  console.log('segment %d (n = %d, true mean %s): mean(mu) = %s  sd(mu) = %s  95%% interval [%s, %s]  mean(sigma) = %s', d, sizes[d], (160 + 0.1 * d).toFixed(1),
    moments[d].mu.mean[0].toFixed(2), moments[d].mu.sd[0].toFixed(3), q[0].toFixed(2), q[1].toFixed(2), moments[d].sigma.mean[0].toFixed(2));
});
console.log('kernel:', sampler.info().launch[0].kernel, ' datasets per launch:', sampler.info().launch[0].datasets);
sampler.close();
