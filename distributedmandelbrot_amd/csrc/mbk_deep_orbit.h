// mbk_deep_orbit.h -- host side of the deep-zoom views (include/mbk.h, "Deep-zoom views"): the reference orbit of a view's
// centre in signed fixed point with P fraction bits, and the decimal parser that reads the centre.  Plain C++, no device
// code, no library (there is no MPFR / GMP dependency): numbers are two's-complement integers X over uint64_t limbs, value
// X / 2^P, limb 0 least significant, the top limb the signed integer part.
//
//   parse    [+-]?digits[.digits]?([eE][+-]?digits)?  ->  X = sign * floor(D * 10^e * 2^P)   (D = all digits as an integer,
//            e = exponent - fraction digits; for e < 0 the scaled D is divided by 10 |e| times, each truncating)
//   product  trunc(a * b / 2^P): magnitudes multiplied, shifted right by P, sign restored (truncation toward zero)
//   orbit    Z_0 = 0, Z_{k+1} = (sr - si + Cr, 2 t + Ci) with sr = trunc(Zr Zr), si = trunc(Zi Zi), t = trunc(Zr Zi);
//            stop at the first M with trunc(Zr Zr) + trunc(Zi Zi) >= 4 (of Z_M), or at M = mrd; each Z_k rounded to
//            nearest-even binary64 (subnormals included), and beside it as a binary64 mantissa pair with one int32 exponent
//            (the wide table: no Z_k but 0 itself is lost to the exponent range)
#pragma once

#include <stdint.h>

#include <atomic>
#include <cmath>
#include <string>
#include <vector>

namespace mbk {

constexpr uint32_t kDeepMinBits = 64, kDeepMaxBits = 4096;

// A fixed-point number of n = P / 64 + 1 limbs.
using Fixed = std::vector<uint64_t>;

inline bool fx_negative(const Fixed &a) { return (int64_t)a.back() < 0; }

inline void fx_negate(Fixed &a)
{
    unsigned carry = 1;
    for (uint64_t &w : a) {
        const uint64_t v = ~w + carry;
        carry = (carry && v == 0) ? 1u : 0u;
        w = v;
    }
}

inline Fixed fx_add(const Fixed &a, const Fixed &b)
{
    Fixed r(a.size());
    unsigned __int128 carry = 0;
    for (size_t k = 0; k < a.size(); ++k) {
        const unsigned __int128 s = (unsigned __int128)a[k] + b[k] + carry;
        r[k] = (uint64_t)s;
        carry = s >> 64;
    }
    return r;
}

inline Fixed fx_sub(const Fixed &a, const Fixed &b)
{
    Fixed nb = b;
    fx_negate(nb);
    return fx_add(a, nb);
}

// trunc(a * b / 2^P), P = 64 (n - 1)
inline Fixed fx_mul(const Fixed &a, const Fixed &b)
{
    const size_t n = a.size();
    const bool neg = fx_negative(a) != fx_negative(b);
    Fixed ma = a, mb = b;
    if (fx_negative(ma)) fx_negate(ma);
    if (fx_negative(mb)) fx_negate(mb);
    std::vector<uint64_t> prod(2 * n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (ma[i] == 0) continue;
        unsigned __int128 carry = 0;
        for (size_t j = 0; j < n; ++j) {
            const unsigned __int128 t = (unsigned __int128)ma[i] * mb[j] + prod[i + j] + carry;
            prod[i + j] = (uint64_t)t;
            carry = t >> 64;
        }
        for (size_t k = i + n; carry != 0 && k < 2 * n; ++k) {
            const unsigned __int128 t = (unsigned __int128)prod[k] + carry;
            prod[k] = (uint64_t)t;
            carry = t >> 64;
        }
    }
    Fixed r(prod.begin() + (n - 1), prod.begin() + (2 * n - 1));   // drop P = 64 (n - 1) fraction bits
    if (neg) fx_negate(r);
    return r;
}

// a >= k for a small non-negative integer k
inline bool fx_ge_int(const Fixed &a, uint64_t k)
{
    if (fx_negative(a)) return false;
    return a.back() >= k;   // integer part >= k, the fraction is >= 0
}

// the bit length of |X| (0 for X = 0)
inline int fx_bit_length(const Fixed &a)
{
    Fixed m = a;
    if (fx_negative(m)) fx_negate(m);
    for (int k = (int)m.size() - 1; k >= 0; --k)
        if (m[k]) return 64 * k + (64 - __builtin_clzll(m[k]));
    return 0;
}

// X / 2^P rounded to nearest binary64, ties to even (a subnormal result rounds once, on its own grid)
inline double fx_round(const Fixed &a, int P)
{
    Fixed m = a;
    const bool neg = fx_negative(m);
    if (neg) fx_negate(m);
    int h = 0;   // bit length of |X|
    for (int k = (int)m.size() - 1; k >= 0; --k)
        if (m[k]) {
            h = 64 * k + (64 - __builtin_clzll(m[k]));
            break;
        }
    if (h == 0) return 0.0;
    auto bit = [&](int i) -> uint64_t { return (i >= 0 && i < h) ? (m[i >> 6] >> (i & 63)) & 1u : 0u; };
    const int e = h - 1 - P;                 // exponent of the leading bit
    const int keep = e < -1022 ? 53 - (-1022 - e) : 53;   // significant bits the result can hold
    const int s = h - keep;                  // bits dropped
    if (s <= 0) {                            // exact
        uint64_t v = 0;
        for (int i = 0; i < h; ++i) v |= bit(i) << i;
        const double r = std::ldexp((double)v, -P);
        return neg ? -r : r;
    }
    uint64_t q = 0;
    for (int i = s; i < h; ++i) q |= bit(i) << (i - s);
    const uint64_t rb = bit(s - 1);
    bool sticky = false;
    for (int i = 0; i < s - 1 && !sticky; ++i) sticky = bit(i) != 0;
    if (rb && (sticky || (q & 1u))) ++q;
    const double r = std::ldexp((double)q, s - P);   // q <= 2^53 on its grid: exact
    return neg ? -r : r;
}

// the number itself: X / 2^P with P = 64 (n - 1)
inline double fx_to_double(const Fixed &a) { return fx_round(a, 64 * ((int)a.size() - 1)); }

// ---- decimal parser ----

// Unsigned big integer, little-endian 64-bit limbs, no leading zero limbs.
struct BigU {
    std::vector<uint64_t> w;
    void mul_add(uint64_t mul, uint64_t add)
    {
        unsigned __int128 carry = add;
        for (uint64_t &x : w) {
            const unsigned __int128 t = (unsigned __int128)x * mul + carry;
            x = (uint64_t)t;
            carry = t >> 64;
        }
        if (carry) w.push_back((uint64_t)carry);
    }
    void div10()
    {
        unsigned __int128 rem = 0;
        for (size_t k = w.size(); k-- > 0;) {
            const unsigned __int128 cur = (rem << 64) | w[k];
            w[k] = (uint64_t)(cur / 10u);
            rem = cur % 10u;
        }
        while (!w.empty() && w.back() == 0) w.pop_back();
    }
    bool zero() const { return w.empty(); }
};

// The decimal string as fixed point with P fraction bits (P / 64 + 1 limbs).  False for a malformed string or |x| >= 4.
inline bool fx_parse(const char *s, uint32_t P, Fixed *out, std::string *why)
{
    if (!s) {
        *why = "centre string is NULL";
        return false;
    }
    const std::string txt(s);
    auto bad = [&](const char *what) {
        *why = std::string(what) + ": '" + txt + "'";
        return false;
    };
    auto isdig = [](char c) { return c >= '0' && c <= '9'; };
    const char *p = s;
    bool neg = false;
    if (*p == '+' || *p == '-') neg = *p++ == '-';
    BigU d;
    size_t ndig = 0, nfrac = 0;
    if (!isdig(*p)) return bad("not a decimal number");
    while (isdig(*p)) {
        d.mul_add(10u, (uint64_t)(*p++ - '0'));
        ++ndig;
    }
    if (*p == '.') {
        ++p;
        if (!isdig(*p)) return bad("digits expected after the point");
        while (isdig(*p)) {
            d.mul_add(10u, (uint64_t)(*p++ - '0'));
            ++ndig;
            ++nfrac;
        }
    }
    long long ex = 0;
    if (*p == 'e' || *p == 'E') {
        ++p;
        bool eneg = false;
        if (*p == '+' || *p == '-') eneg = *p++ == '-';
        if (!isdig(*p)) return bad("exponent digits expected");
        while (isdig(*p)) {
            if (ex < 1000000000LL) ex = ex * 10 + (*p - '0');
            ++p;
        }
        if (eneg) ex = -ex;
    }
    if (*p != '\0') return bad("not a decimal number");
    if (ndig > 100000u) return bad("more than 100000 digits");
    while (!d.w.empty() && d.w.back() == 0) d.w.pop_back();
    const size_t n = P / 64u + 1u;
    Fixed r(n, 0ull);
    if (!d.zero()) {
        const long long e10 = ex - (long long)nfrac;
        if (e10 >= 1) return bad("|x| >= 4");
        d.w.insert(d.w.begin(), P / 64u, 0ull);   // D * 2^P
        // D * 2^P < 10^ndig * 2^4096 < 10^(ndig + 1234): after that many divisions nothing is left
        const long long k = -e10;
        if (k > (long long)ndig + 1240) d.w.clear();
        for (long long i = 0; i < k && !d.zero(); ++i) d.div10();
        if (d.w.size() > n || (d.w.size() == n && d.w[n - 1] >= 4u)) return bad("|x| >= 4");
        for (size_t j = 0; j < d.w.size(); ++j) r[j] = d.w[j];
        if (neg) fx_negate(r);
    }
    *out = r;
    return true;
}

// ---- the orbit ----

// One entry of the wide table (mbk.h, "Extended-range deep views"): Z = (xr, xi) 2^xe, the larger |component| in [0.5, 1] (1 when it
// rounds up); a zero Z is (0, 0, kWideZeroExp).  32 bytes, the form the device reads.
constexpr int32_t kWideZeroExp = -(1 << 24);
struct alignas(32) WideEntry {
    double xr, xi;
    int32_t xe;
    int32_t pad[3];
};
static_assert(sizeof(WideEntry) == 32, "the wide table is 32 bytes per entry");

// xe = the bit length of the larger |component| minus P (its frexp exponent); the components over 2^(P + xe), each rounded by
// fx_round -- the smaller one may land in the subnormal range and then rounds once, on that grid.
inline WideEntry fx_to_wide(const Fixed &zr, const Fixed &zi)
{
    const int P = 64 * ((int)zr.size() - 1);
    const int hr = fx_bit_length(zr), hi = fx_bit_length(zi);
    const int H = hr > hi ? hr : hi;
    if (H == 0) return WideEntry{0.0, 0.0, kWideZeroExp, {0, 0, 0}};
    return WideEntry{fx_round(zr, H), fx_round(zi, H), H - P, {0, 0, 0}};
}

struct DeepOrbit {
    uint64_t id;                 // never reused: the key of each ctx's device copy
    uint32_t precision_bits;     // P
    uint32_t mrd;                // the orbit was computed up to M <= mrd
    uint32_t length;             // M
    uint32_t escaped;            // 1 iff |Z_M|^2 >= 4
    std::vector<double> table;   // (Zr, Zi, 2 Zr, 2 Zi) for k = 0 .. M: the 32 bytes per entry the kernel reads
    std::vector<WideEntry> wide; // Z_k = (xr, xi) 2^xe for k = 0 .. M: what the wide kernel reads (mbk_deep_wide.h)
};

inline uint64_t next_orbit_id()
{
    static std::atomic<uint64_t> counter{0};
    return ++counter;
}

inline bool build_deep_orbit(const char *cr, const char *ci, uint32_t P, uint32_t mrd, DeepOrbit *o, std::string *why)
{
    if (P < kDeepMinBits || P > kDeepMaxBits || P % 64u != 0u) {
        *why = "precision_bits must be a multiple of 64 in [64, 4096]";
        return false;
    }
    if (mrd < 2u || mrd > 0x7fffffffu) {
        *why = "orbit mrd must lie in [2, 2^31 - 1]";
        return false;
    }
    Fixed Cr, Ci;
    if (!fx_parse(cr, P, &Cr, why) || !fx_parse(ci, P, &Ci, why)) return false;
    const size_t n = P / 64u + 1u;
    Fixed zr(n, 0ull), zi(n, 0ull);
    o->precision_bits = P;
    o->mrd = mrd;
    o->escaped = 0u;
    o->table.assign(4, 0.0);   // Z_0 = 0
    o->wide.assign(1, WideEntry{0.0, 0.0, kWideZeroExp, {0, 0, 0}});
    uint32_t k = 0;
    while (true) {
        const Fixed sr = fx_mul(zr, zr), si = fx_mul(zi, zi), t = fx_mul(zr, zi);
        if (k > 0 && fx_ge_int(fx_add(sr, si), 4u)) {
            o->escaped = 1u;
            break;
        }
        if (k == mrd) break;
        zr = fx_add(fx_sub(sr, si), Cr);
        zi = fx_add(fx_add(t, t), Ci);
        ++k;
        const double dr = fx_to_double(zr), di = fx_to_double(zi);
        o->table.push_back(dr);
        o->table.push_back(di);
        o->table.push_back(dr + dr);
        o->table.push_back(di + di);
        o->wide.push_back(fx_to_wide(zr, zi));
    }
    o->length = k;
    o->id = next_orbit_id();
    return true;
}

}  // namespace mbk
