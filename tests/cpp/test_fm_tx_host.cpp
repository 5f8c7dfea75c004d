// test_fm_tx_host.cpp — VectorSource -> FmTx -> VectorSink under the C++ host mirror's Graph (rustradio_amd/host/rustradio.hpp):
// the modulator of examples/fm_tx.rs:84-91 against the reference's recurrence (src/vco.rs:24-36) restated here in double.
// Needs a GPU.  Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_fm_tx_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cmath>
#include <cstdio>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

int main() {
    const size_t n_in = 5000, interp = 10, deci = 1, n = n_in * interp / deci;
    const double k = 2.0 * M_PI * 5000.0 / 480000.0;       // fm_tx.rs:88-90 at its default rates
    std::vector<Float> audio(n_in);
    for (size_t i = 0; i < n_in; i++) audio[i] = (Float)(0.8 * std::sin(2.0 * M_PI * 1000.0 / 48000.0 * (double)i));

    auto [src, s0] = VectorSource<Float>::new_(audio);
    auto [tx, s1] = FmTx::new_(std::move(s0), interp, deci, k);
    CHECK(std::string(tx->block_name()) == "RationalResampler>Vco");
    auto sink = std::make_unique<VectorSink<Complex>>(std::move(s1));
    auto hook = sink->hook();
    Graph g;
    g.add(std::move(src)); g.add(std::move(tx)); g.add(std::move(sink));
    g.run();
    CHECK(hook->size() == n);

    // the model: phase += k * a once per OUTPUT sample, one wrap by MX, (sin, cos)
    const double MX = 2.0 * M_PI;
    std::vector<double> ms(n), mc(n);
    double phase = 0.0;
    for (size_t m = 0; m < n; m++) {
        phase += k * (double)audio[m * deci / interp];
        if (phase > MX) phase -= MX;
        if (phase < -MX) phase += MX;
        ms[m] = std::sin(phase); mc[m] = std::cos(phase);
    }
    // both sides' distance to the truth: half an f32 ulp of the cast plus the phase error of either sum
    const double tol = std::ldexp(1.0, -24) + 2.0 * ((double)n * std::ldexp(1.0, -48));
    double worst = 0;
    if (hook->size() == n)
        for (size_t j = 0; j < 32; j++) {
            const size_t m = j < 16 ? j : n - 32 + j;
            const Complex y = (*hook)[m];
            worst = std::max(worst, std::max(std::fabs((double)y.real() - ms[m]), std::fabs((double)y.imag() - mc[m])));   // re = sin
        }
    printf("worst %.4e, allowed %.4e\n", worst, tol);
    CHECK(worst <= tol);

    // Vco::new_ alone is a sync block of the mirror: the same stream through RationalResampler -> Vco
    {
        auto [src2, a0] = VectorSource<Float>::new_(audio);
        auto [rs, a1] = RationalResampler<Float>::new_(std::move(a0), interp, deci);
        auto [vco, a2] = Vco::new_(std::move(a1), k);
        CHECK(std::string(vco->block_name()) == "Vco");
        auto sink2 = std::make_unique<VectorSink<Complex>>(std::move(a2));
        auto hook2 = sink2->hook();
        Graph g2;
        g2.add(std::move(src2)); g2.add(std::move(rs)); g2.add(std::move(vco)); g2.add(std::move(sink2));
        g2.run();
        CHECK(hook2->size() == n);
        double w2 = 0;
        if (hook2->size() == n)
            for (size_t m = n - 16; m < n; m++)
                w2 = std::max(w2, std::max(std::fabs((double)(*hook2)[m].real() - ms[m]), std::fabs((double)(*hook2)[m].imag() - mc[m])));
        CHECK(w2 <= tol);
    }
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
