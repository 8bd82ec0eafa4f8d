'use strict';
// A logistic regression per segment on 64 segments at once: one posterior per segment, 256 chains each, ONE sampler and one launch per call.  The closure ends in the
// logistic-regression loop, so the translated dataset sampler keeps its certified decisions (kernel amwg_user_step_cert_ds, 16 lanes per chain): every segment's chains are
// the reference's, bit for bit, at more than twice the rate of evaluating the expression in every update.  The segments must be of EQUAL SHAPE (here: 400 rows each):
//   node examples/logit_datasets.js
const { mcmc, ld } = require('../bayes.js_amd');
global.ld = ld;

var params = {
  b: {type: "real", dim: [3], init: 0}};

var log_post = function(state, data) {
  var lp = 0;
  for (var j = 0; j < 3; j++) lp += ld.norm(state.b[j], 0, 10);
  for (var i = 0; i < data.y.length; i++) {
    var eta = state.b[0] + state.b[1] * data.x1[i] + state.b[2] * data.x2[i];
    lp += data.y[i] * eta - Math.log1p(Math.exp(eta));
  }
  return lp;
};

// 64 synthetic segments of 400 rows; the effect of x1 differs per segment
var datasets = [];
for (var d = 0; d < 64; d++) {
  var x1 = [], x2 = [], y = [];
  for (var i = 0; i < 400; i++) {
    var a = mcmc.runif(-2, 2), c = mcmc.runif(-1, 1);
    x1.push(a); x2.push(c);
    y.push(mcmc.runif(0, 1) < 1 / (1 + Math.exp(-(0.3 + (0.2 + 0.02 * d) * a - 0.6 * c))) ? 1 : 0);
  }
  datasets.push({ x1: x1, x2: x2, y: y });
}

// the data argument is null: options.datasets takes its place; options.chains is the total
var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, translate: true, chains: 64 * 256, seed: 1 });
sampler.burn(1000);
sampler.sample(200);
var moments = sampler.dataset_moments();
var quant = sampler.dataset_quantiles([0.025, 0.975]);      // a 95 % credible interval per segment, selected on the device
var cov = sampler.dataset_covariance(['b']);                // the coefficient covariance and correlation per segment, formed on the device
[0, 1, 32, 63].forEach(function (d) {
  var q = quant[d].b[1];
  console.log('segment %d (true effect of x1 %s): mean(b[1]) = %s  sd = %s  95%% interval [%s, %s]', d, (0.2 + 0.02 * d).toFixed(2),
    moments[d].b.mean[1].toFixed(3), moments[d].b.sd[1].toFixed(3), q[0].toFixed(3), q[1].toFixed(3));
  console.log('  correlation of %s:', cov[d].labels.join(', '));
  cov[d].cor.forEach(function (row) { console.log('   ', row.map(function (v) { return v.toFixed(3); }).join('  ')); });
});
var launch = sampler.info().launch[0];
console.log('kernel:', launch.kernel, ' lanes per chain:', launch.lanes_per_chain, ' summation order:', launch.summation_order, ' datasets per launch:', launch.datasets);
sampler.close();
