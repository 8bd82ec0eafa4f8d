'use strict';
// A closure NO built-in family recognises -- a robust regression line per segment: Student-t errors around a + b * x, and the derived quantity "predicted y at x = 1" --
// on 64 segments at once: one posterior per segment, 256 chains each, ONE sampler and one launch per call.  options.datasets takes the segments, and
// options.translate: true asks for the translated dataset sampler: every segment is translated and all must give one source, so the segments must be of EQUAL SHAPE
// (here: 200 points each; the values are free):
//   node examples/closure_datasets.js
const { mcmc, ld } = require('../bayes.js_amd');
global.ld = ld;

var params = {
  a: {type: "real"},
  b: {type: "real"},
  sigma: {type: "real", lower: 0}};

var log_post = function(state, data) {
  var lp = ld.norm(state.a, 0, 100) + ld.norm(state.b, 0, 100) + ld.unif(state.sigma, 0, 100);
  for (var i = 0; i < data.x.length; i++) {
    lp += ld.t((data.y[i] - (state.a + state.b * data.x[i])) / state.sigma, 0, 1, data.df) - Math.log(state.sigma);
  }
  state.y_at_1 = state.a + state.b;
  return lp;
};

// 64 synthetic segments of 200 points; the true slope differs per segment, every tenth point is an outlier.  `df` is a scalar field of the data: it is the same in every
// segment here and is folded into the source; a scalar that differed between the segments would be read at run time instead
var datasets = [];
for (var d = 0; d < 64; d++) {
  var x = [], y = [];
  for (var i = 0; i < 200; i++) {
    var xi = mcmc.runif(-2, 2);
    x.push(xi);
    y.push(1 + (0.5 + 0.02 * d) * xi + mcmc.rnorm(0, i % 10 === 0 ? 5 : 0.5));
  }
  datasets.push({ x: x, y: y, df: 4 });
}

// the data argument is null: options.datasets takes its place; options.chains is the total
var sampler = new mcmc.AmwgSampler(params, log_post, null, { datasets: datasets, translate: true, chains: 64 * 256, seed: 1 });
sampler.burn(1000);
sampler.sample(200);
var moments = sampler.dataset_moments();
var quant = sampler.dataset_quantiles([0.025, 0.975]);      // a 95 % credible interval per segment, selected on the device
[0, 1, 32, 63].forEach(function (d) {
  var q = quant[d].b[0], p = quant[d].y_at_1[0];
  console.log('segment %d (true slope %s): mean(b) = %s  sd(b) = %s  95%% interval [%s, %s]  y at x = 1: %s [%s, %s]', d, (0.5 + 0.02 * d).toFixed(2),
    moments[d].b.mean[0].toFixed(3), moments[d].b.sd[0].toFixed(3), q[0].toFixed(3), q[1].toFixed(3), moments[d].y_at_1.mean[0].toFixed(3), p[0].toFixed(3), p[1].toFixed(3));
});
console.log('kernel:', sampler.info().launch[0].kernel, ' datasets per launch:', sampler.info().launch[0].datasets);
sampler.close();
