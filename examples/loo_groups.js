'use strict';
// Leave-one-group-out beside leave-one-out: a hierarchical model written as a plain closure -- eight schools with a mean each, drawn from a common distribution --,
// translated (options.translate) with its pointwise terms (options.pointwise).  loo() asks how well the model predicts ONE MORE MEASUREMENT of a school it knows;
// loo({groups: g}) leaves out a whole school at a time: the importance ratio of a draw for school k is exp(-sum of the school's terms), formed on the device as
// a sum over the school's observations in index order, and everything after that -- the Pareto fit, khat, the totals -- is the rule of loo() with schools for
// observations.  Expect elpd per school well below the sum of its observations' elpd_loo_i (its own mean is no longer informed by its data) and larger khat.
//   node examples/loo_groups.js
const { mcmc, ld } = require('../bayes.js_amd');
global.ld = ld;

var params = {
  theta: {type: "real", dim: [8], init: 0},
  mu: {type: "real"},
  sigma: {type: "real", lower: 0}};

var log_post = function(state, data) {
  var log_post = 0;
  log_post += ld.norm(state.mu, 0, 10);
  log_post += ld.unif(state.sigma, 0, 20);
  for (var k = 0; k < 8; k++) log_post += ld.norm(state.theta[k], state.mu, 3);
  for (var i = 0; i < data.y.length; i++) {
    log_post += ld.norm(data.y[i], state.theta[data.g[i]], state.sigma);
  }
  return log_post;
};

// 8 schools of unequal size, 200 pupils in all; school k's mean is k / 2 - 2
var y = [], g = [];
for (var i = 0; i < 200; i++) {
  var k = Math.min(7, Math.floor(8 * Math.pow(i / 200, 1.6)));
  g.push(k);
  y.push(mcmc.rnorm(k / 2 - 2, 1.5));
}

var sampler = new mcmc.AmwgSampler(params, log_post, { y: y, g: g }, { translate: true, pointwise: true, chains: 1024, seed: 1 });
sampler.burn(2000);
sampler.sample_on_device(200);
var one = sampler.loo({ pointwise: true }), school = sampler.loo({ groups: g, pointwise: true });
var f = function (v) { return v.toFixed(2); };
console.log('leave-one-out:       elpd_loo %s +- %s, p_loo %s, khat > 0.7 at %d of %d observations', f(one.elpd_loo), f(one.se), f(one.p_loo), one.high_k, one.pointwise.length);
console.log('leave-one-group-out: elpd_loo %s +- %s, p_loo %s, khat > 0.7 at %d of %d schools', f(school.elpd_loo), f(school.se), f(school.p_loo), school.high_k, school.n_groups);
school.pointwise.forEach(function (t, k) {
  var own = 0, n = 0;
  for (var i = 0; i < g.length; i++) if (g[i] === k) { own += one.pointwise[i][0]; n++; }
  console.log('  school %d (%d pupils): left out whole %s (khat %s)   its pupils left out one by one %s', k, n, f(t[0]), f(t[2]), f(own));
});
sampler.close();
