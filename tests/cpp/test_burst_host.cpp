// test_burst_host.cpp — VectorSource<Complex> -> BurstDetector -> VectorSink under the C++ host mirror's Graph
// (rustradio_amd/host/rustradio.hpp): the reference's own expectation for BurstTagger (src/burst_tagger.rs tag_it) — the samples
// pass through unchanged, and the tags are the source's three plus (80, "burst", true) and (90, "burst", false).  With alpha 1
// the filtered power IS the power, 0.0625 during the burst and 0 elsewhere, so the crossings of 0.03 are exact.
// Needs a GPU.  Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_burst_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static bool has(const std::vector<Tag>& v, const Tag& t) { return std::find(v.begin(), v.end(), t) != v.end(); }

int main() {
    std::vector<Complex> z(100, Complex(0, 0));
    for (size_t i = 80; i < 90; i++) z[i] = Complex(0.25f, 0);
    for (size_t i = 0; i < 100; i++) if (i < 80 || i >= 90) z[i] = Complex(0, (Float)i * 1e-3f);   // distinct samples, power <= 0.0099

    auto [src, s0] = VectorSource<Complex>::new_(z);
    auto [det, s1] = BurstDetector::new_(std::move(s0), 1.0f, 0.03f, "burst");
    CHECK(std::string(det->block_name()) == "ComplexToMag2>SinglePoleIirFilter>BurstTagger");
    auto sink = std::make_unique<VectorSink<Complex>>(std::move(s1));
    auto hook = sink->hook();
    auto tags = sink->tag_hook();
    Graph g;
    g.add(std::move(src)); g.add(std::move(det)); g.add(std::move(sink));
    g.run();
    CHECK(*hook == z);
    CHECK(tags->size() == 5);
    CHECK(has(*tags, Tag(0, "VectorSource::start", true)));
    CHECK(has(*tags, Tag(0, "VectorSource::first", true)));
    CHECK(has(*tags, Tag(0, "VectorSource::repeat", (uint64_t)0)));
    CHECK(has(*tags, Tag(80, "burst", true)));
    CHECK(has(*tags, Tag(90, "burst", false)));
    for (auto& t : *tags) printf("tag %zu %s\n", t.pos(), t.key().c_str());

    // SinglePoleIirFilter::new_ is the reference's Option; ComplexToMag2 and the filter are sync blocks of the mirror
    for (Float bad : {-0.1f, 1.1f, std::nanf("")}) {
        auto [srcb, b0] = VectorSource<Float>::new_(std::vector<Float>{0.1f, 0.2f});
        CHECK(!SinglePoleIirFilter<Float>::new_(std::move(b0), bad).has_value());
    }
    {
        auto [src2, a0] = VectorSource<Complex>::new_(z);
        auto [m2, a1] = ComplexToMag2::new_(std::move(a0));
        auto iir = SinglePoleIirFilter<Float>::new_(std::move(a1), 1.0f);
        CHECK(iir.has_value());
        if (iir) {
            CHECK(std::string(m2->block_name()) == "ComplexToMag2" && std::string(iir->first->block_name()) == "SinglePoleIirFilter");
            auto sink2 = std::make_unique<VectorSink<Float>>(std::move(iir->second));
            auto hook2 = sink2->hook();
            Graph g2;
            g2.add(std::move(src2)); g2.add(std::move(m2)); g2.add(std::move(iir->first)); g2.add(std::move(sink2));
            g2.run();
            CHECK(hook2->size() == 100);
            if (hook2->size() == 100) {
                CHECK((*hook2)[85] == 0.0625f && (*hook2)[79] == z[79].imag() * z[79].imag() && (*hook2)[0] == 0.0f);
            }
        }
    }
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
