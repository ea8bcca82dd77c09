// gd_round3g.hpp -- what `%.3g` prints for a float32, without formatting any text: the three
// significant decimal digits and the decimal exponent of the first of them.
//
// indexcov prints every cell of its BED matrix with fmt.Sprintf("%.3g", depth) on a float32
// (indexcov/indexcov.go depthsFor).  Go's strconv converts with bit size 32: the digits are the EXACT
// binary value of the float32 rounded to three significant digits, ties to even.  So a cell is a pure
// function of the bits of x = m * 2^q (m < 2^24):
//   x * 10^j = m * 5^j * 2^(q + j)          (j >= 0: x < 1000)       an integer shifted right
//   x / 10^k = m * 2^q / 10^k               (k  > 0: x >= 1000)      an integer quotient
// Both are evaluated in integers -- a 134-bit product in three 64-bit words for the smallest
// subnormal -- and the remainder decides the rounding: no floating-point operation takes part, so
// there is nothing a compiler could contract, and the host and the device instance are one text.
// Domain: 0 <= x < 1e9 (indexcov caps depths at 50 000); x >= 1e9, infinities and NaN give digits 0.
//
// The result packs digits d (100 .. 999, or 0 for x == 0) and the exponent e (x ~ d / 100 * 10^e) as
// d | (uint32_t)(e + 128) << 16.  gd_fmt3g() turns that into the text Go prints: fixed notation for
// e in -4 .. 2 with the trailing zeros of the fraction dropped, else d.dde+XX (50 000 -> "5e+04").
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GD3_HD __host__ __device__ inline
#else
#define GD3_HD inline
#endif

// floor(x * 10^j), the half bit and the sticky bit of the rest, for x = m * 2^q, j >= 0, x * 10^j < 2^62.
GD3_HD uint64_t gd3_scale_up(uint32_t m, int q, int j, bool* half, bool* sticky)
{
    uint64_t lo = 1, hi = 0;                              // 5^j, j <= 47: below 2^110
    for (int i = 0; i < j; ++i) {
        const uint64_t l4 = lo << 2, h4 = (hi << 2) | (lo >> 62);
        const uint64_t nl = l4 + lo;
        hi = h4 + hi + (nl < l4 ? 1u : 0u);
        lo = nl;
    }
    // L2:L1:L0 = m * (hi:lo)
    const uint64_t p0 = (uint64_t)m * (lo & 0xffffffffu), p1 = (uint64_t)m * (lo >> 32);
    const uint64_t p2 = (uint64_t)m * (hi & 0xffffffffu), p3 = (uint64_t)m * (hi >> 32);
    uint64_t L0 = p0 + (p1 << 32);
    uint64_t c = L0 < p0 ? 1u : 0u;
    uint64_t L1 = (p1 >> 32) + c;                          // < 2^25
    uint64_t t = L1 + p2;                                  // p2 < 2^56: no carry
    L1 = t + (p3 << 32);
    c = L1 < t ? 1u : 0u;
    uint64_t L2 = (p3 >> 32) + c;
    const int s = -(q + j);                                // the value is L * 2^-s
    *half = false;
    *sticky = false;
    if (s <= 0) return L0 << (-s);                         // (an integer below 2^62 by the precondition)
    int n = s - 1;                                         // shift to the half bit
    bool lost = false;
    if (n >= 128) { lost = (L0 | L1) != 0; L0 = L2; L1 = 0; L2 = 0; n -= 128; }
    else if (n >= 64) { lost = L0 != 0; L0 = L1; L1 = L2; L2 = 0; n -= 64; }
    if (n > 0) {
        lost = lost || (L0 & ((1ull << n) - 1)) != 0;
        L0 = (L0 >> n) | (L1 << (64 - n));
    }
    *half = (L0 & 1u) != 0;
    *sticky = lost;
    return L0 >> 1;
}

// floor(x / 10^k), half and sticky, for x = m * 2^q, 1000 <= x < 1e9, 1 <= k <= 6.
GD3_HD uint64_t gd3_scale_down(uint32_t m, int q, int k, bool* half, bool* sticky)
{
    uint64_t num = m, den = 1;
    for (int i = 0; i < k; ++i) den *= 10;
    if (q >= 0) num <<= q; else den <<= -q;                // x >= 1000: q >= -14; x < 2^30: q <= 6
    const uint64_t d = num / den, r2 = (num - d * den) * 2;
    *half = r2 >= den;
    *sticky = r2 != den && r2 != 0;
    if (*half && r2 == den) *sticky = false;
    return d;
}

GD3_HD uint32_t gd_round3g(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    u &= 0x7fffffffu;                                      // (depths are not negative)
    if (u == 0 || u >= 0x4e6e6b28u) return 0;              // 0, or >= 1e9 / inf / NaN
    const int be = (int)(u >> 23);
    const uint32_t m = be ? (u & 0x7fffffu) | 0x800000u : (u & 0x7fffffu);
    const int q = (be ? be : 1) - 150;
    // the position of the leading bit gives the decimal exponent to within one
    int top = 23;
    while (!((m >> top) & 1u)) --top;
    const int E = q + top;                                 // floor(log2 x)
    int e = (E * 78913) >> 18;                             // floor(E * log10(2)); the true exponent is e or e + 1
    uint64_t d = 0;
    for (int pass = 0; pass < 2; ++pass) {
        bool half, sticky;
        const int j = 2 - e;
        const uint64_t f = j >= 0 ? gd3_scale_up(m, q, j, &half, &sticky) : gd3_scale_down(m, q, -j, &half, &sticky);
        if (f >= 1000) { ++e; continue; }                  // (only in the first pass)
        d = f;
        if (half && (sticky || (d & 1u))) ++d;             // ties to even on the exact value
        break;
    }
    if (d >= 1000) { d = 100; ++e; }
    return (uint32_t)d | ((uint32_t)(e + 128) << 16);
}

// The text of one packed cell; returns its length (at most 9 bytes, no terminator).
inline int gd_fmt3g(uint32_t cell, char* out)
{
    const int d = (int)(cell & 0xffffu), e = (int)(cell >> 16) - 128;
    if (d == 0) { out[0] = '0'; return 1; }
    char dig[3] = {(char)('0' + d / 100), (char)('0' + d / 10 % 10), (char)('0' + d % 10)};
    int nd = 3;
    while (nd > 1 && dig[nd - 1] == '0') --nd;             // strconv's digits carry no trailing zeros
    int n = 0;
    if (e < -4 || e >= 3) {                                // %e: d[.dd]e+XX
        out[n++] = dig[0];
        if (nd > 1) { out[n++] = '.'; for (int i = 1; i < nd; ++i) out[n++] = dig[i]; }
        out[n++] = 'e';
        int a = e;
        if (a < 0) { out[n++] = '-'; a = -a; } else out[n++] = '+';
        out[n++] = (char)('0' + a / 10);
        out[n++] = (char)('0' + a % 10);
        return n;
    }
    if (e >= 0) {                                          // e + 1 integer digits
        for (int i = 0; i <= e; ++i) out[n++] = i < nd ? dig[i] : '0';
        if (nd > e + 1) { out[n++] = '.'; for (int i = e + 1; i < nd; ++i) out[n++] = dig[i]; }
        return n;
    }
    out[n++] = '0';
    out[n++] = '.';
    for (int i = 0; i < -e - 1; ++i) out[n++] = '0';
    for (int i = 0; i < nd; ++i) out[n++] = dig[i];
    return n;
}
