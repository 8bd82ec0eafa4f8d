"""Where the polynomial pieces of csrc/amwg_cdf.h come from: Chebyshev fits (mpmath, 60 digits) of
    A  erf(x) / x          in t = x^2 - 1/8          on 0 <= x < 1/2
    B  erfcx(x)            in t = x - 1              on 1/2 <= x < 3/2
    C  erfcx(x)            in t = x - 9/4            on 3/2 <= x < 3
    D  x erfcx(x)          in t = 1/x^2 - 5/72       on 3 <= x < 6
    E  x erfcx(x)          in t = 1/x^2 - 1/64       on 6 <= x <= 28      (erfcx(x) = exp(x^2) erfc(x))
each of the lowest degree whose fit error is below 2^-57 of the function.  Prints the arrays as the header holds them, highest power first (Horner).
Run by hand when a piece changes; nothing at build or test time reads it."""
import mpmath as mp

mp.mp.dps = 60


def erfcx(x):
    return mp.exp(x * x) * mp.erfc(x)


PIECES = [
    ("A", lambda t: mp.erf(mp.sqrt(t + mp.mpf(1) / 8)) / mp.sqrt(t + mp.mpf(1) / 8), -mp.mpf(1) / 8 + mp.mpf(10) ** -40, mp.mpf(1) / 8),
    ("B", lambda t: erfcx(t + 1), -mp.mpf(1) / 2, mp.mpf(1) / 2),
    ("C", lambda t: erfcx(t + mp.mpf(9) / 4), -mp.mpf(3) / 4, mp.mpf(3) / 4),
    ("D", lambda t: erfcx(1 / mp.sqrt(t + mp.mpf(5) / 72)) / mp.sqrt(t + mp.mpf(5) / 72), mp.mpf(1) / 36 - mp.mpf(5) / 72, mp.mpf(1) / 9 - mp.mpf(5) / 72),
    ("E", lambda t: erfcx(1 / mp.sqrt(t + mp.mpf(1) / 64)) / mp.sqrt(t + mp.mpf(1) / 64), mp.mpf(1) / 784 - mp.mpf(1) / 64, mp.mpf(1) / 36 - mp.mpf(1) / 64),
]

if __name__ == "__main__":
    for name, f, a, b in PIECES:
        floor = min(abs(f(a)), abs(f(b)))
        for n in range(6, 40):
            coeffs, err = mp.chebyfit(f, [a, b], n, error=True)
            if err < floor * mp.mpf(2) ** -57:
                break
        print("// piece %s: degree %d, fit error %.2g of the function" % (name, n - 1, float(err / floor)))
        print("constexpr double k%s[%d] = {%s};" % (name, n, ", ".join(float(c).hex() for c in coeffs)))
