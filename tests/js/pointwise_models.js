// (sloppy mode on purpose, as user_models.js: the closures are written the way a bayes.js user writes them, against a global `ld`)
/*
 * pointwise_models.js -- TEST FIXTURES for options.pointwise (WAIC and PSIS-LOO of translated closures): closures whose observations are the iterations of their
 * final loop.  Each case gives log_post AND, written separately, what the pointwise plan must reproduce:
 *   head(state, data)      the closure up to its final loop (the prior: no part of the terms)
 *   term(state, data, i)   the double the final loop's `acc += term` adds in iteration i
 * so that head + the sequential sum of term(i) is log_post, bit for bit (tests/js/pointwise_cli.js checks that first, under V8).
 * data(n, seed): n observations.  REJECTED: closures the plan must refuse, each with a fragment of its pointwise_why.
 */
function lcg(seed) { let s = seed >>> 0; return () => { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; }; }
function gauss(r) { return (r() + r() + r() + r() - 2) * 1.7320508; }

const CASES = {};

// ---- README.md:18-43: the Normal family's twin (real-valued heights, so that the family stores the same doubles)
CASES.normal = {
  params: () => ({ mu: { type: 'real' }, sigma: { type: 'real', lower: 0 } }),
  data: (n, seed) => { const r = lcg(seed), x = []; for (let i = 0; i < n; i++) x.push(180 + 6 * gauss(r)); return x; },
  state: (r) => ({ mu: 180 + 3 * gauss(r), sigma: 1 + 9 * r() }),
  log_post: function(state, data) {
    var log_post = 0;
    log_post += ld.norm(state.mu, 0, 100);
    log_post += ld.unif(state.sigma, 0, 100);
    for(var i = 0; i < data.length; i++) {
      log_post += ld.norm(data[i], state.mu, state.sigma);
    }
    return log_post;
  },
  head: function(state, data) { var lp = 0; lp += ld.norm(state.mu, 0, 100); lp += ld.unif(state.sigma, 0, 100); return lp; },
  term: function(state, data, i) { return ld.norm(data[i], state.mu, state.sigma); },
  twin: 'normal',
};

// ---- README.md:149-164: a Bernoulli loop (at one lane per chain the step kernel fast-forwards it; the terms are those of the plain loop)
CASES.bern = {
  params: () => ({ theta: { type: 'real', lower: 0, upper: 1 } }),
  data: (n, seed) => { const r = lcg(seed), x = []; for (let i = 0; i < n; i++) x.push(r() < 0.3 ? 1 : 0); return x; },
  state: (r) => ({ theta: 0.02 + 0.96 * r() }),
  log_post: function(state, data) {
    var log_post = 0;
    log_post += ld.beta(state.theta, 2, 2);
    for(var i = 0; i < data.length; i++) {
      log_post += ld.bern(data[i], state.theta);
    }
    return log_post;
  },
  head: function(state, data) { var lp = 0; lp += ld.beta(state.theta, 2, 2); return lp; },
  term: function(state, data, i) { return ld.bern(data[i], state.theta); },
  twin: 'beta_bern',
};

// ---- group means gathered by a label: theta[g[i]] (the hierarchical family's twin: theta[0 .. G - 1], mu, sigma)
CASES.hier = {
  G: 5,
  params: () => ({ theta: { type: 'real', dim: [5], init: 0 }, mu: { type: 'real' }, sigma: { type: 'real', lower: 0 } }),
  data: (n, seed) => { const r = lcg(seed), y = [], g = []; for (let i = 0; i < n; i++) { g.push(i % 5 === 4 ? Math.floor(r() * 5) : i % 5); y.push(g[i] - 2 + 1.5 * gauss(r)); } return { y, g }; },
  state: (r) => ({ theta: [0, 1, 2, 3, 4].map((k) => k - 2 + 0.5 * gauss(r)), mu: 0.3 * gauss(r), sigma: 0.5 + 2 * r() }),
  log_post: function(state, data) {
    var lp = 0;
    lp += ld.norm(state.mu, 0, 10);
    lp += ld.unif(state.sigma, 0, 20);
    for (var k = 0; k < 5; k++) lp += ld.norm(state.theta[k], state.mu, 3);
    for (var i = 0; i < data.y.length; i++) {
      lp += ld.norm(data.y[i], state.theta[data.g[i]], state.sigma);
    }
    return lp;
  },
  head: function(state, data) { var lp = 0; lp += ld.norm(state.mu, 0, 10); lp += ld.unif(state.sigma, 0, 20); for (var k = 0; k < 5; k++) lp += ld.norm(state.theta[k], state.mu, 3); return lp; },
  term: function(state, data, i) { return ld.norm(data.y[i], state.theta[data.g[i]], state.sigma); },
  twin: 'hier_normal',
};

// ---- the Poisson regression with a change point (the Poisson family's twin: beta[0 .. 7], cp)
CASES.pois_glm = {
  params: (d) => ({ beta: { type: 'real', dim: [8], init: 0 }, cp: { type: 'int', lower: 0, upper: Math.max(1, d.y.length - 1) } }),
  data: (n, seed) => {
    const r = lcg(seed), X = [], y = [];
    for (let i = 0; i < n; i++) { X.push(1); for (let k = 1; k < 7; k++) X.push(0.5 * gauss(r)); y.push(Math.floor(r() * 6)); }
    return { X, y };
  },
  state: (r, d) => ({ beta: [0, 1, 2, 3, 4, 5, 6, 7].map(() => 0.3 * gauss(r)), cp: Math.floor(r() * d.y.length) }),
  log_post: function(s, d) {
    var lp = 0;
    for (var k = 0; k < 8; k++) lp += ld.norm(s.beta[k], 0, 10);
    lp += ld.unif(s.cp, 0, 1000);
    for (var i = 0; i < d.y.length; i++) {
      var eta = d.X[i * 7] * s.beta[0];
      eta += d.X[i * 7 + 1] * s.beta[1];
      eta += d.X[i * 7 + 2] * s.beta[2];
      eta += d.X[i * 7 + 3] * s.beta[3];
      eta += d.X[i * 7 + 4] * s.beta[4];
      eta += d.X[i * 7 + 5] * s.beta[5];
      eta += d.X[i * 7 + 6] * s.beta[6];
      if (i >= s.cp) eta += s.beta[7];
      lp += ld.pois(d.y[i], Math.exp(eta));
    }
    return lp;
  },
  head: function(s, d) { var lp = 0; for (var k = 0; k < 8; k++) lp += ld.norm(s.beta[k], 0, 10); lp += ld.unif(s.cp, 0, 1000); return lp; },
  term: function(s, d, i) {
    var eta = d.X[i * 7] * s.beta[0];
    for (var k = 1; k < 7; k++) eta += d.X[i * 7 + k] * s.beta[k];
    if (i >= s.cp) eta += s.beta[7];
    return ld.pois(d.y[i], Math.exp(eta));
  },
  twin: 'pois_glm',
};

// ---- logistic regression through Math.log1p(Math.exp(eta)); some rows push |eta| far beyond what the step loop's open softplus covers
CASES.logistic = {
  params: () => ({ b0: { type: 'real' }, b1: { type: 'real' } }),
  data: (n, seed) => { const r = lcg(seed), x = [], y = []; for (let i = 0; i < n; i++) { x.push(i % 7 === 3 ? (r() < 0.5 ? -1 : 1) * (300 + 600 * r()) : 2 * gauss(r)); y.push(r() < 0.5 ? 1 : 0); } return { x, y }; },
  state: (r) => ({ b0: gauss(r), b1: 1.5 * gauss(r) }),
  log_post: function(state, data) {
    var lp = ld.norm(state.b0, 0, 5) + ld.norm(state.b1, 0, 5);
    for (var i = 0; i < data.x.length; i++) {
      var eta = state.b0 + state.b1 * data.x[i];
      lp += data.y[i] * eta - Math.log1p(Math.exp(eta));
    }
    return lp;
  },
  head: function(state, data) { return ld.norm(state.b0, 0, 5) + ld.norm(state.b1, 0, 5); },
  term: function(state, data, i) { var eta = state.b0 + state.b1 * data.x[i]; return data.y[i] * eta - Math.log1p(Math.exp(eta)); },
};

// ---- several statements with private locals in the body
CASES.locals = {
  params: () => ({ a: { type: 'real' }, b: { type: 'real' }, ls: { type: 'real' }, c: { type: 'real' } }),
  data: (n, seed) => { const r = lcg(seed), x = [], z = [], y = []; for (let i = 0; i < n; i++) { x.push(gauss(r)); z.push(r()); y.push(1 + 2 * x[i] + gauss(r)); } return { x, z, y }; },
  state: (r) => ({ a: 1 + 0.3 * gauss(r), b: 2 + 0.3 * gauss(r), ls: 0.2 * gauss(r), c: 0.4 * gauss(r) }),
  log_post: function(state, data) {
    var lp = 0;
    lp += ld.norm(state.a, 0, 10);
    lp += ld.norm(state.b, 0, 10);
    lp += ld.norm(state.ls, 0, 2);
    lp += ld.norm(state.c, 0, 2);
    for (var i = 0; i < data.y.length; i++) {
      var m = state.a + state.b * data.x[i];
      var s = Math.exp(state.ls + state.c * data.z[i]);
      var r = (data.y[i] - m) / s;
      lp += -0.5 * r * r - Math.log(s);
    }
    return lp;
  },
  head: function(state, data) { var lp = 0; lp += ld.norm(state.a, 0, 10); lp += ld.norm(state.b, 0, 10); lp += ld.norm(state.ls, 0, 2); lp += ld.norm(state.c, 0, 2); return lp; },
  term: function(state, data, i) { var m = state.a + state.b * data.x[i]; var s = Math.exp(state.ls + state.c * data.z[i]); var r = (data.y[i] - m) / s; return -0.5 * r * r - Math.log(s); },
};

// ---- the loop uses a local computed in the head
CASES.head_local = {
  params: () => ({ mu: { type: 'real' }, ls: { type: 'real' } }),
  data: (n, seed) => { const r = lcg(seed), y = []; for (let i = 0; i < n; i++) y.push(3 + 2 * gauss(r)); return { y }; },
  state: (r) => ({ mu: 3 + gauss(r), ls: 0.5 * gauss(r) }),
  log_post: function(state, data) {
    var lp = 0;
    var sd = Math.exp(state.ls);
    lp += ld.norm(state.mu, 0, 10);
    lp += ld.norm(state.ls, 0, 3);
    for (var i = 0; i < data.y.length; i++) lp += ld.norm(data.y[i], state.mu, sd);
    return lp;
  },
  head: function(state, data) { var lp = 0; lp += ld.norm(state.mu, 0, 10); lp += ld.norm(state.ls, 0, 3); return lp; },
  term: function(state, data, i) { return ld.norm(data.y[i], state.mu, Math.exp(state.ls)); },
};

// ---- a derived quantity (written in the head) and an int parameter
CASES.derived_int = {
  params: () => ({ rate: { type: 'real', lower: 0, init: 2 }, k: { type: 'int', lower: 0, upper: 6, init: 2 } }),
  data: (n, seed) => { const r = lcg(seed), y = []; for (let i = 0; i < n; i++) y.push(Math.floor(r() * 9)); return { y }; },
  state: (r) => ({ rate: 0.5 + 3 * r(), k: Math.floor(r() * 7) }),
  log_post: function(state, data) {
    var lp = 0;
    lp += ld.gamma(state.rate, 2, 1);
    lp += ld.unif(state.k, 0, 6);
    state.scaled = state.rate * (1 + state.k);
    for (var i = 0; i < data.y.length; i++) lp += ld.pois(data.y[i], state.rate * (1 + state.k));
    return lp;
  },
  head: function(state, data) { var lp = 0; lp += ld.gamma(state.rate, 2, 1); lp += ld.unif(state.k, 0, 6); return lp; },
  term: function(state, data, i) { return ld.pois(data.y[i], state.rate * (1 + state.k)); },
};

// ---- 40 state entries read as theta[i % 40]: a Draw that holds the whole state, large enough to shorten the staged run
CASES.wide_state = {
  params: () => ({ theta: { type: 'real', dim: [40], init: 0 } }),
  data: (n, seed) => { const r = lcg(seed), y = []; for (let i = 0; i < n; i++) y.push(gauss(r)); return { y }; },
  state: (r) => ({ theta: Array.from({ length: 40 }, () => 0.7 * gauss(r)) }),
  log_post: function(state, data) {
    var lp = 0;
    for (var k = 0; k < 40; k++) lp += ld.norm(state.theta[k], 0, 2);
    for (var i = 0; i < data.y.length; i++) lp += ld.norm(data.y[i], state.theta[i % 40], 1.5);
    return lp;
  },
  head: function(state, data) { var lp = 0; for (var k = 0; k < 40; k++) lp += ld.norm(state.theta[k], 0, 2); return lp; },
  term: function(state, data, i) { return ld.norm(data.y[i], state.theta[i % 40], 1.5); },
};

// ---- one observation whose term is -Infinity under every draw (a negative count): observation min(3, n - 1)
CASES.minus_inf = {
  params: () => ({ lr: { type: 'real' } }),
  data: (n, seed) => { const r = lcg(seed), y = []; for (let i = 0; i < n; i++) y.push(Math.floor(r() * 7)); y[Math.min(3, n - 1)] = -1; return { y }; },
  state: (r) => ({ lr: 1 + 0.4 * gauss(r) }),
  log_post: function(state, data) {
    var lp = 0;
    lp += ld.norm(state.lr, 0, 3);
    var rate = Math.exp(state.lr);
    for (var i = 0; i < data.y.length; i++) lp += ld.pois(data.y[i], rate);
    return lp;
  },
  head: function(state, data) { var lp = 0; lp += ld.norm(state.lr, 0, 3); return lp; },
  term: function(state, data, i) { return ld.pois(data.y[i], Math.exp(state.lr)); },
  bad_obs: (n) => Math.min(3, n - 1),
};

// ---- closures the plan refuses, each by its reason
const REJECTED = {
  loop_not_last: {
    why: 'is not a loop',
    params: () => ({ mu: { type: 'real' } }),
    data: (n, seed) => CASES.head_local.data(n, seed),
    log_post: function(state, data) {
      var lp = 0;
      for (var i = 0; i < data.y.length; i++) lp += ld.norm(data.y[i], state.mu, 2);
      lp += ld.norm(state.mu, 0, 10);
      return lp;
    },
  },
  acc_twice: {
    why: 'more than once',
    params: () => ({ mu: { type: 'real' } }),
    data: (n, seed) => CASES.head_local.data(n, seed),
    log_post: function(state, data) {
      var lp = 0;
      lp += ld.norm(state.mu, 0, 10);
      for (var i = 0; i < data.y.length; i++) { lp += ld.norm(data.y[i], state.mu, 2); lp += -0.001 * data.y[i] * data.y[i]; }
      return lp;
    },
  },
  has_break: {
    why: 'has a break',
    params: () => ({ mu: { type: 'real' } }),
    data: (n, seed) => CASES.head_local.data(n, seed),
    log_post: function(state, data) {
      var lp = 0;
      lp += ld.norm(state.mu, 0, 10);
      for (var i = 0; i < data.y.length; i++) { if (data.y[i] > 1e6) break; lp += ld.norm(data.y[i], state.mu, 2); }
      return lp;
    },
  },
  early_return: {
    why: 'returns early',
    params: () => ({ mu: { type: 'real' } }),
    data: (n, seed) => CASES.head_local.data(n, seed),
    log_post: function(state, data) {
      var lp = 0;
      if (state.mu > 1e3) return -Infinity;
      lp += ld.norm(state.mu, 0, 10);
      for (var i = 0; i < data.y.length; i++) lp += ld.norm(data.y[i], state.mu, 2);
      return lp;
    },
  },
  under_if: {
    why: 'under a conditional',
    params: () => ({ mu: { type: 'real' } }),
    data: (n, seed) => CASES.head_local.data(n, seed),
    log_post: function(state, data) {
      var lp = 0;
      lp += ld.norm(state.mu, 0, 10);
      if (state.mu > -50) {
        for (var i = 0; i < data.y.length; i++) lp += ld.norm(data.y[i], state.mu, 2);
      }
      return lp;
    },
  },
  derived_in_loop: {
    why: 'derived quantity',      // (the translator refuses such a closure altogether: its own sentence)
    params: () => ({ mu: { type: 'real' } }),
    data: (n, seed) => CASES.head_local.data(n, seed),
    log_post: function(state, data) {
      var lp = 0;
      lp += ld.norm(state.mu, 0, 10);
      for (var i = 0; i < data.y.length; i++) { state.last = data.y[i] - state.mu; lp += ld.norm(data.y[i], state.mu, 2); }
      return lp;
    },
  },
};

// (not a matter of the loop's form: the whole state of 1 600 entries would have to be kept per draw, 12 808 bytes, and fewer than four of those fit the staged run)
REJECTED.draw_too_large = {
  why: 'fewer than 4 of those fit',
  params: () => ({ theta: { type: 'real', dim: [1600], init: 0 } }),
  data: (n, seed) => CASES.head_local.data(n, seed),
  log_post: function(state, data) {
    var lp = 0;
    for (var k = 0; k < 1600; k++) lp += ld.norm(state.theta[k], 0, 2);
    for (var i = 0; i < data.y.length; i++) lp += ld.norm(data.y[i], state.theta[i % 1600], 1.5);
    return lp;
  },
};

function build(name, n, seed) {
  const c = CASES[name] || REJECTED[name];
  if (!c) throw new Error('unknown pointwise model ' + name);
  const data = c.data(n === undefined ? 65 : n, seed === undefined ? 20261021 : seed);
  return { name, params: c.params(data), log_post: c.log_post, head: c.head, term: c.term, state: c.state, data, why: c.why, twin: c.twin, bad_obs: c.bad_obs };
}

module.exports = { CASES, REJECTED, build, names: Object.keys(CASES), rejected: Object.keys(REJECTED), lcg };
