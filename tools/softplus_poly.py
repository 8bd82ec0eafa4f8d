"""Coefficients of softplus_bounded (bayes.js_amd/csrc/amwg_math.h SoftplusLiterals): log1p(t) = 2 atanh(s) = 2 s + s z Q(z), s = t / (2 + t) in (0, 1/3],
z = s s in (0, 1/9], Q(z) = 2 (1/3 + z/5 + z^2/7 + ...).  Q is replaced by the polynomial of degree 9 that interpolates it at the ten Chebyshev nodes of
[0, 1/9 (1 + 1e-6)] (50-digit arithmetic), converted to the monomial basis and rounded to doubles.  Prints the doubles and the distance of 2 s + s z Q(z) from
log1p(t) in EXACT arithmetic on a grid of t in (0, 1] -- what is left of softplus_bounded's error is exp_bounded's and the roundings.
python tools/softplus_poly.py"""
import mpmath as mp
mp.mp.dps = 50
N = 10      # degree 9 interpolant: 10 nodes
hi = mp.mpf(1) / 9 * (1 + mp.mpf("1e-6"))


def Q(z):
    if z == 0:
        return mp.mpf(2) / 3
    r = mp.sqrt(z)
    return (2 * mp.atanh(r) / r - 2) / z


nodes = [mp.cos((2 * j + 1) * mp.pi / (2 * N)) for j in range(N)]
f = [Q(hi * (t + 1) / 2) for t in nodes]
c = [sum(f[j] * mp.chebyt(k, nodes[j]) for j in range(N)) * 2 / N for k in range(N)]
c[0] /= 2
# sum c_k T_k(t), t = 2 z / hi - 1, in the monomial basis of z
polys = [[mp.mpf(1)], [mp.mpf(0), mp.mpf(1)]]
for k in range(2, N):
    p = [mp.mpf(0)] + [2 * v for v in polys[k - 1]]
    q = polys[k - 2] + [mp.mpf(0)] * (len(p) - len(polys[k - 2]))
    polys.append([p[i] - q[i] for i in range(len(p))])
mono_t = [mp.mpf(0)] * N
for k in range(N):
    for i, v in enumerate(polys[k]):
        mono_t[i] += c[k] * v
coef = [mp.mpf(0)] * N      # t^i = (2 z / hi - 1)^i
for i, v in enumerate(mono_t):
    for j in range(i + 1):
        coef[j] += v * mp.binomial(i, j) * (2 / hi) ** j * (-1) ** (i - j)
for i, v in enumerate(coef):
    print(i, float(v).hex(), float(v), "x %d / 2 = %.16g" % (2 * i + 3, float(v * (2 * i + 3) / 2)))
cd = [mp.mpf(float(v)) for v in coef]      # the coefficients as the doubles they become
worst = mp.mpf(0)
for k in range(1, 8001):
    t = mp.mpf(k) / 8000
    s = t / (2 + t)
    z = s * s
    p = mp.mpf(0)
    for v in reversed(cd):
        p = p * z + v
    worst = max(worst, abs(2 * s + s * z * p - mp.log1p(t)))
print("max absolute distance from log1p on (0, 1], double coefficients, exact arithmetic:", float(worst))
print("constexpr double " + ", ".join("q%d = %s" % (i, float(coef[i]).hex()) for i in range(N)) + ";")
