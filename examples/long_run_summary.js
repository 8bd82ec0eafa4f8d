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
// a short pilot places the edges of a histogram: 1 024 uniform bins over the pilot's central 99.8 % widened by its own span on either side
sampler.sample_on_device(500);
var pilot = sampler.quantiles([0.001, 0.999]), edges = {}, bins = 1024;
for (const name of ['mu', 'sigma']) {
  const lo = pilot[name][0][0], hi = pilot[name][0][1], a = lo - (hi - lo), w = 3 * (hi - lo) / bins;
  edges[name] = Array.from({ length: bins + 1 }, (_, i) => a + i * w);
}
// the long run counts its draws under those edges while they pass: the 95 % interval of the stored run's quantiles() lies inside the brackets printed below
// ... and folds the co-moment of mu and sigma beside the fold of each window: a correlation for a run that kept no draw
// ... and the lagged sums of each chain at lags 0 .. 100: the integrated autocorrelation time tau and an ESS that looks along the chains, beside the between-chain one
var kept = sampler.summarize(200000, { histogram: edges, covariance: true, autocorrelation: { max_lag: 100 } });
var m = sampler.moments(), c = sampler.convergence(), h = sampler.histogram(), cv = sampler.covariance(), ac = sampler.autocorrelation();
console.log('kept draws per chain:', kept);
for (const name of ['mu', 'sigma']) {
  const b = mcmc.interval_brackets(h[name][0], edges[name], [0.025, 0.975]);
  const k = ac.labels.indexOf(name);
  console.log('%s: mean %s  sd %s  R-hat %s  ESS %s  tau %s  autocorrelation ESS %s%s  2.5 %% in [%s, %s]  97.5 %% in [%s, %s]', name, m[name].mean[0].toFixed(3), m[name].sd[0].toFixed(3),
              c[name].rhat[0].toFixed(5), c[name].ess[0].toFixed(0), ac.tau[k].toFixed(2), ac.ess[k].toFixed(0), ac.truncated[k] ? '' : ' (an upper bound: ask for more lags)',
              b[0][0].toFixed(3), b[0][1].toFixed(3), b[1][0].toFixed(3), b[1][1].toFixed(3));
}
console.log('cor(%s, %s) = %s  (cov %s)', cv.labels[0], cv.labels[1], cv.cor[0][1].toFixed(4), cv.cov[0][1].toExponential(3));
console.log('held on the device:', JSON.stringify(sampler.summary_info()));
sampler.close();
