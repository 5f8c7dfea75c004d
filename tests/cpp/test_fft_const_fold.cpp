// The 8- and 16-point butterflies of rustradio_amd/csrc/fft_core.hpp (host forms), forward and inverse, against a direct
// O(R^2) DFT in double: the 2 R unit impulses (each position, re and im) and 64 seeded random vectors per transform.
// Next to them runs the unfolded form of the same butterflies (every constant rotation w16^m as a product of its own, the
// way the butterflies were written before the rotations' real factors moved into the FMAs): the folded ones have to stay
// within TOL and within one f32 rounding of the unfolded ones' worst error.
// Build: g++ -std=c++17 -fsanitize=address,undefined -I rustradio_amd/csrc tests/cpp/test_fft_const_fold.cpp
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>

#include "fft_core.hpp"

using namespace rr;

namespace unfolded {
constexpr float kC = 0.92387953251128675613f, kS = 0.38268343236508977173f, kH = 0.70710678118654752440f;
cf scale(cf a, float k) { return mk(a.x * k, a.y * k); }
cf mul(cf a, cf b) { return mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
cf mulc(cf a, cf b) { return mk(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
// a * w16^m (forward) or its conjugate, m in {1, 2, 3, 4, 6, 9}
template <bool INV> cf mul_w16(cf a, int m) {
    const cf zero = mk(0.0f, 0.0f);
    if (m == 4) return add_w4<INV>(zero, a);
    if (m == 2) return scale(add_w4<INV>(a, a), kH);
    if (m == 6) return scale(sub_w4<INV>(a, a), -kH);
    const float c = m == 1 ? kC : m == 3 ? kS : -kC, s = m == 1 ? kS : m == 3 ? kC : -kS;
    return INV ? mulc(a, mk(c, -s)) : mul(a, mk(c, -s));
}
template <bool INV> void dft8(cf* v) {
    bfly4<INV>(v[0], v[2], v[4], v[6]);
    bfly4<INV>(v[1], v[3], v[5], v[7]);
    v[3] = mul_w16<INV>(v[3], 2); v[5] = mul_w16<INV>(v[5], 4); v[7] = mul_w16<INV>(v[7], 6);
    bfly2<INV>(v[0], v[1]); bfly2<INV>(v[2], v[3]); bfly2<INV>(v[4], v[5]); bfly2<INV>(v[6], v[7]);
    cf o[8];
    for (int k1 = 0; k1 < 4; k1++) for (int k2 = 0; k2 < 2; k2++) o[k1 + 4 * k2] = v[2 * k1 + k2];
    for (int i = 0; i < 8; i++) v[i] = o[i];
}
template <bool INV> void dft16(cf* v) {
    for (int n2 = 0; n2 < 4; n2++) bfly4<INV>(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
    for (int k1 = 1; k1 < 4; k1++) for (int n2 = 1; n2 < 4; n2++) v[4 * k1 + n2] = mul_w16<INV>(v[4 * k1 + n2], k1 * n2);
    for (int k1 = 0; k1 < 4; k1++) bfly4<INV>(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
    cf o[16];
    for (int k1 = 0; k1 < 4; k1++) for (int k2 = 0; k2 < 4; k2++) o[k1 + 4 * k2] = v[4 * k1 + k2];
    for (int i = 0; i < 16; i++) v[i] = o[i];
}
}  // namespace unfolded

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static float uniform() {   // (-1, 1), splitmix64
    uint64_t z = (g_seed += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (float)((double)(z >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

constexpr double TOL = 1e-5;                 // the project's bound, relative to the output's max
constexpr double ONE_ROUNDING = 5.9604644775390625e-8;   // 2^-24: one f32 operation, relative to its result

// max |got - want| / max |want|
template <int R> double rel_err(const cf* got, const std::complex<double>* want) {
    double e = 0, m = 0;
    for (int k = 0; k < R; k++) {
        e = fmax(e, std::abs(std::complex<double>(got[k].x, got[k].y) - want[k]));
        m = fmax(m, std::abs(want[k]));
    }
    return e / m;
}

template <int R, bool INV> int run() {
    double worst_new = 0, worst_old = 0, worst_impulse = 0;
    for (int c = 0; c < 2 * R + 64; c++) {
        cf x[R], a[R], b[R];
        for (int i = 0; i < R; i++) {
            if (c < 2 * R) x[i] = mk(c == i ? 1.0f : 0.0f, c == R + i ? 1.0f : 0.0f);
            else x[i] = mk(uniform(), uniform());
            a[i] = b[i] = x[i];
        }
        std::complex<double> want[R];
        for (int k = 0; k < R; k++) {
            std::complex<double> s = 0;
            for (int n = 0; n < R; n++)
                s += std::complex<double>(x[n].x, x[n].y) * std::polar(1.0, (INV ? 2.0 : -2.0) * M_PI * ((k * n) % R) / R);
            want[k] = s;
        }
        Dft<R, INV>::run(a);
        if (R == 8) unfolded::dft8<INV>(b); else unfolded::dft16<INV>(b);
        const double en = rel_err<R>(a, want), eo = rel_err<R>(b, want);
        worst_new = fmax(worst_new, en);
        worst_old = fmax(worst_old, eo);
        if (c < 2 * R) worst_impulse = fmax(worst_impulse, en);
    }
    const bool ok = worst_new <= TOL && worst_new <= worst_old + ONE_ROUNDING;
    printf("dft%-2d %s  worst err / max: folded %.3e  unfolded %.3e  (folded, impulses only %.3e)  %s\n", R, INV ? "inverse" : "forward",
           worst_new, worst_old, worst_impulse, ok ? "ok" : "FAIL");
    return ok ? 0 : 1;
}

int main() {
    int f = run<8, false>() + run<8, true>() + run<16, false>() + run<16, true>();
    printf(f ? "FAIL %d\n" : "fft const fold ok\n", f);
    return f ? 1 : 0;
}
