'use strict';
// Is the README model (README.md:18-43) CALIBRATED on heavy-tailed data?  5-fold in ONE launch: the five training folds are the datasets of one ragged sampler, and
// dataset_predictive() gives every held-out observation its probability integral transform (PIT), predictive mean and predictive sd on the device.  The data are
// Student-t with 2 degrees of freedom: a Normal likelihood answers the tails with a large sigma, so far MORE than half of the observations land in its central 50 %
// interval and the PIT histogram piles up in the middle.  elpd alone would not say where the model is wrong; this does.
//   node examples/calibration.js
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

// 200 heights with heavy tails: 170 + 7 t_2, t_2 = z / sqrt(chi2_2 / 2)
var K = 5, x = [];
for (var i = 0; i < 200; i++) {
  var z = mcmc.rnorm(0, 1), a = mcmc.rnorm(0, 1), b = mcmc.rnorm(0, 1);
  x.push(170 + 7 * z / Math.sqrt((a * a + b * b) / 2));
}
var test = [], train = [];
for (var k = 0; k < K; k++) {
  test.push(x.filter(function (_, i) { return i % K === k; }));
  train.push(x.filter(function (_, i) { return i % K !== k; }));
}

var folds = new mcmc.AmwgSampler(params, log_post, null, { datasets: train, chains: K * 1024, seed: 1 });
folds.burn(1000);
folds.sample_on_device(250);
var held = folds.dataset_predictive({ data: test }), own = folds.dataset_predictive({ pointwise: false });
folds.close();

var all = [].concat.apply([], held.map(function (f) { return f.pointwise; }));
var inside = function (lo, hi) { return all.filter(function (p) { var m = (p.pit_hi + p.pit_lo) / 2; return lo <= m && m <= hi; }).length / all.length; };
var f = function (v) { return v.toFixed(2); };
console.log('held-out (5 folds): ' + f(100 * inside(0.25, 0.75)) + ' % of the observations in the central 50 % interval, ' + f(100 * inside(0.05, 0.95)) + ' % in the 90 % interval');
console.log('in-sample (optimistic), fold 0: ' + f(100 * own[0].cover50) + ' % and ' + f(100 * own[0].cover90) + ' %; held-out rmse of fold 0: ' + f(held[0].rmse));
console.log('PIT histogram, 10 bins (a calibrated model: ' + all.length / 10 + ' each): ' + mcmc.pit_histogram(all, 10).join(' '));
