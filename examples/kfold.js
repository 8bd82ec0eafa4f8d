'use strict';
// 5-fold cross-validation of the README model (README.md:18-43) in ONE launch: the five training folds are the datasets of one ragged sampler (options.datasets),
// and dataset_heldout() scores every fold's stored draws on the observations that fold has not seen, on the device.  The sample holds ONE PLANTED OUTLIER: loo() of
// the full fit reports it (khat above 0.7: high_k) and cannot repair it; K-fold does not lean on importance sampling, so elpd_kfold is the number to trust there.
//   node examples/kfold.js
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

// 100 heights; one is 60 cm off
var K = 5, x = [];
for (var i = 0; i < 100; i++) x.push(mcmc.rnorm(170, 7));
x[42] += 60;
// the folds, dealt round-robin: fold k is scored on the observations i with i % K == k by the fit of all the others
var test = [], train = [];
for (var k = 0; k < K; k++) {
  test.push(x.filter(function (_, i) { return i % K === k; }));
  train.push(x.filter(function (_, i) { return i % K !== k; }));
}

var folds = new mcmc.AmwgSampler(params, log_post, null, { datasets: train, chains: K * 1024, seed: 1 });
folds.burn(1000);
folds.sample_on_device(250);
var total = mcmc.kfold_total(folds.dataset_heldout(test, { pointwise: true }));
folds.close();

var full = new mcmc.AmwgSampler(params, log_post, x, { chains: 1024, seed: 1 });
full.burn(1000);
full.sample_on_device(250);
var loo = full.loo({ pointwise: true });
full.close();

var f = function (v) { return v.toFixed(2); };
console.log('elpd_kfold ' + f(total.elpd_kfold) + ' +- ' + f(total.se) + ' over ' + total.n + ' observations in ' + K + ' folds');
console.log('elpd_loo   ' + f(loo.elpd_loo) + ' +- ' + f(loo.se) + ', ' + loo.high_k + ' observation(s) with khat > 0.7 (khat of the outlier: ' + f(loo.pointwise[42][2]) + ')');
