'use strict';
// logit_models.js -- TEST FIXTURES: closures that end in a logistic-regression loop, for the certified logistic tail (bayes.js_amd/translate.js glmTailPlan,
// csrc/amwg_gtail.h) on and off its fast path, and the closures for which the translator must NOT emit that plan.  Kept apart from user_models.js, whose closures
// have goldens of the reference; these are compared with the same closure at one lane per chain with the expression in every update.
//   build(name, n, ymode) -> { params, data, log_post }     n observations (default 517: a ragged last round); ymode 'zeros' | 'ones' | undefined (drawn)
const { lcg } = require('./user_models.js');

// x1 in [-2, 2) with x1[0] = 2 and x1[1] = -2 exactly (a start state b[1] = B puts max |eta| at 2 B whatever n is), x2 in [-1, 1), labels g in {0, 1, 2},
// weights w in (0, 3) with a few negative ones, y in {0, 1} drawn from the model
function data(n, seed, ymode) {
  const r = lcg(seed === undefined ? 20261016 : seed), x1 = [], x2 = [], g = [], w = [], y = [];
  for (let i = 0; i < n; i++) {
    const a = i === 0 ? 2 : i === 1 ? -2 : r() * 4 - 2, b = r() * 2 - 1;
    x1.push(a); x2.push(b); g.push(Math.floor(r() * 3)); w.push(i % 37 === 5 ? -0.75 * r() : 3 * r());
    const p = 1 / (1 + Math.exp(-(0.3 + 0.9 * a - 0.6 * b)));
    y.push(ymode === 'zeros' ? 0 : ymode === 'ones' ? 1 : (r() < p ? 1 : 0));
  }
  return { x1, x2, g, w, y };
}

const params = () => ({ b: { dim: [4], init: 0 } });
const CASES = {
  // the fast path: every state index a constant (scalar-register state), every data read of the observation's own row (row cache)
  logit_tail_small: function (s, d) {
    var lp = 0;
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    for (var i = 0; i < d.y.length; i++) {
      var eta = s.b[0] + s.b[1] * d.x1[i] + s.b[2] * d.x2[i];
      lp += d.y[i] * eta - Math.log1p(Math.exp(eta));
    }
    return lp;
  },
  // a coefficient gathered by the data: per-lane reads of the state, the plain loop
  logit_tail_gather: function (s, d) {
    var lp = 0;
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    for (var i = 0; i < d.y.length; i++) {
      var eta = s.b[d.g[i]] * 0.5 + s.b[3] * d.x1[i];
      lp += d.y[i] * eta - Math.log1p(Math.exp(eta));
    }
    return lp;
  },
  // a read of the NEXT observation's row: scalar-register state, no row cache
  logit_tail_next_row: function (s, d) {
    var lp = 0;
    const N = d.y.length;
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    for (var i = 0; i < N; i++) {
      var eta = s.b[0] + d.x1[(i + 1) % N] * s.b[1] + d.x2[i] * s.b[2];
      lp += d.y[i] * eta - Math.log1p(Math.exp(eta));
    }
    return lp;
  },
  // real-valued weights in the place of y (the product rounds), eta as the first factor
  logit_tail_weights: function (s, d) {
    var lp = 0;
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    for (var i = 0; i < d.w.length; i++) {
      var eta = s.b[0] + s.b[1] * d.x1[i] + s.b[3] * d.x2[i];
      lp += eta * d.w[i] - Math.log1p(Math.exp(eta));
    }
    return lp;
  },
  // ---- no plan: the loop followed by another statement; a derived quantity; eta differs in the two places
  logit_not_last: function (s, d) {
    var lp = 0;
    for (var i = 0; i < d.y.length; i++) {
      var eta = s.b[0] + s.b[1] * d.x1[i];
      lp += d.y[i] * eta - Math.log1p(Math.exp(eta));
    }
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    return lp;
  },
  logit_derived: function (s, d) {
    var lp = 0;
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    s.odds = Math.exp(s.b[1]);
    for (var i = 0; i < d.y.length; i++) {
      var eta = s.b[0] + s.b[1] * d.x1[i];
      lp += d.y[i] * eta - Math.log1p(Math.exp(eta));
    }
    return lp;
  },
  logit_two_etas: function (s, d) {
    var lp = 0;
    for (var j = 0; j < 4; j++) lp += ld.norm(s.b[j], 0, 10);
    for (var i = 0; i < d.y.length; i++) {
      var eta = s.b[0] + s.b[1] * d.x1[i], eta2 = s.b[0] + s.b[2] * d.x2[i];
      lp += d.y[i] * eta - Math.log1p(Math.exp(eta2));
    }
    return lp;
  },
};

function build(name, n, ymode) {
  if (!CASES[name]) throw new Error('unknown logit fixture ' + name);
  return { name, params: params(), data: data(n || 517, undefined, ymode), log_post: CASES[name] };
}

module.exports = { CASES, build, data, params, names: Object.keys(CASES) };
