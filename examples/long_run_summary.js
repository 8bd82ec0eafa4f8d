'use strict';
// A long run summarised without storing it: the README model on 4 096 chains, 200 000 kept draws per chain.  Stored, the draws would be
// 200 000 x 2 x 4 096 x 8 bytes = 13 GB on the device; summarize() passes them through a window of 64 MiB and keeps six doubles per chain and value.
//   node examples/long_run_summary.js
const { mcmc, ld } = require('../bayes.js_amd');
global.ld = ld;

// The heights of the last ten American presidents in cm, from Kennedy to Obama
var data = [183, 192, 182, 183, 177, 185, 188, 188, 182, 185];

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

var sampler = new mcmc.AmwgSampler(params, log_post, data, { chains: 4096, seed: 1 });
sampler.burn(1000);
var kept = sampler.summarize(200000);
var m = sampler.moments(), c = sampler.convergence();
console.log('kept draws per chain:', kept);
for (const name of ['mu', 'sigma'])
  console.log('%s: mean %s  sd %s  R-hat %s  ESS %s', name, m[name].mean[0].toFixed(3), m[name].sd[0].toFixed(3), c[name].rhat[0].toFixed(5), c[name].ess[0].toFixed(0));
console.log('held on the device:', JSON.stringify(sampler.summary_info()));
sampler.close();
