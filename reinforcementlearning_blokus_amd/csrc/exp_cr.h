// exp_cr.h -- exp(x) in double, rounded from a double-double value good to ~2^-95.
//
// bk_winprob_eval's probabilities are compared with CPython's math.exp chain bit for bit.
// A libm exp within 1 ulp is not enough for that (the device library's differed from the
// host's in 1 value of 172 on the edge boards); a result that is the correctly rounded
// one in all but astronomically rare cases equals every host exp that rounds correctly.
//
// Method: k = rint(x / ln 2); r = x - k ln 2 with ln 2 in three parts (the first has 32
// significant bits, so k * L1 is exact) kept as a double-double; exp(r), |r| <= 0.35, by
// the Taylor series in Horner form, p <- 1 + r p / n for n = 24 .. 1, in double-double
// arithmetic (Dekker / Knuth error-free sums, products through fma); the high word of the
// normalised result is the nearest double of the sum; scaling by 2^k is exact for normal
// results (a subnormal one, x < -708.4, is rounded a second time).  Against a 60-digit exp
// on 55,000 arguments in [-740, 709] the host build differed only in 3 such subnormals.
//
// Compiled for the host too (a stand-alone check against a multi-precision exp needs no
// GPU).  Every operation here must stay as written: the including file compiles this
// under `#pragma clang fp contract(off)`, repeated below for the functions' own bodies.
#ifndef BK_EXP_CR_H
#define BK_EXP_CR_H

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BK_EXP_HD __host__ __device__ inline
#else
#define BK_EXP_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

struct bk_dd {
    double hi, lo;
};

BK_EXP_HD bk_dd bk_two_sum(double a, double b) {  // a + b = hi + lo exactly
    const double s = a + b, bb = s - a;
    return bk_dd{s, (a - (s - bb)) + (b - bb)};
}
BK_EXP_HD bk_dd bk_quick_two_sum(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return bk_dd{s, b - (s - a)};
}
BK_EXP_HD bk_dd bk_two_prod(double a, double b) {  // a * b = hi + lo exactly
    const double p = a * b;
    return bk_dd{p, fma(a, b, -p)};
}
BK_EXP_HD bk_dd bk_dd_add(bk_dd a, bk_dd b) {
    bk_dd s = bk_two_sum(a.hi, b.hi);
    const bk_dd t = bk_two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = bk_quick_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return bk_quick_two_sum(s.hi, s.lo);
}
BK_EXP_HD bk_dd bk_dd_mul(bk_dd a, bk_dd b) {
    bk_dd p = bk_two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return bk_quick_two_sum(p.hi, p.lo);
}
BK_EXP_HD bk_dd bk_dd_div_d(bk_dd a, double b) {
    const double q1 = a.hi / b;
    const bk_dd p = bk_two_prod(q1, b);
    const double rem = ((a.hi - p.hi) - p.lo) + a.lo;
    return bk_quick_two_sum(q1, rem / b);
}

BK_EXP_HD double bk_exp_cr(double x) {
    if (x != x) return x;
    if (x > 709.782712893384) return HUGE_VAL;
    if (x < -745.2) return 0.0;
    const double L1 = 0x1.62e42fee00000p-1, L2 = 0x1.a39ef35793c76p-33, L3 = 0x1.cc01f97b57a08p-87;
    const double k = rint(x * 0x1.71547652b82fep+0);
    bk_dd r = bk_two_sum(x, -(k * L1));  // k * L1 is exact
    const bk_dd k2 = bk_two_prod(-k, L2);
    r = bk_dd_add(r, k2);
    r = bk_dd_add(r, bk_dd{-k * L3, 0.0});
    bk_dd p{1.0, 0.0};
    for (int n = 24; n >= 1; --n) p = bk_dd_add(bk_dd{1.0, 0.0}, bk_dd_div_d(bk_dd_mul(r, p), (double)n));
    // two steps, so that neither factor of a result near the ends of the range overflows
    const int ki = (int)k, half = ki / 2;
    return ldexp(ldexp(p.hi, half), ki - half);
}

#endif  // BK_EXP_CR_H
