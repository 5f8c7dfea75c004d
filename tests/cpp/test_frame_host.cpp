// test_frame_host.cpp — the transmit chain under the C++ host mirror (rustradio_amd/host/rustradio.hpp): HdlcFramer<Float>
// (FcsAdder -> HdlcFramer -> PduToStream -> Scrambler::g3ruh -> NrziEncode -> Map) -> VectorSource -> FmTx -> VectorSink, as
// examples/g3ruh.rs:250-267 wires it, and the same bits through HdlcFramer<uint8_t> -> Scrambler -> NrziEncode as sync blocks.
// Reads the packets tests/test_gpu_frame_host_cpp.py wrote, writes the levels and the Complex stream back for it to judge
// against tests/tx_model.py.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_frame_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>
#include <cstring>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

template <class T> static bool rd(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s packets.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint64_t interp = 0, deci = 0, npk = 0;
    double k = 0;
    float lo = 0, hi = 0;
    CHECK(rd(f, &interp) && rd(f, &deci) && rd(f, &k) && rd(f, &lo) && rd(f, &hi) && rd(f, &npk));
    std::vector<std::vector<uint8_t>> packets(npk);
    for (auto& p : packets) {
        uint64_t n = 0;
        CHECK(rd(f, &n));
        p.resize(n);
        if (n) CHECK(rd(f, p.data(), n));
    }
    std::fclose(f);

    const int flags = RR_FRAME_FCS | RR_FRAME_G3RUH | RR_FRAME_NRZI;
    // two pushes: the register and the level are carried
    const size_t half = packets.size() / 2;
    const std::vector<std::vector<uint8_t>> first(packets.begin(), packets.begin() + (long)half), second(packets.begin() + (long)half, packets.end());
    HdlcFramer<Float> fr(flags, lo, hi);
    CHECK(fr.tile_bits() == 4096);
    auto a = fr.push(first);
    auto b = fr.push(second);
    CHECK(a.records.size() == first.size() && b.records.size() == second.size() && a.tags.size() == first.size());
    if (!a.records.empty()) {
        CHECK(a.tags[0].pos() == 0 && a.tags[0].key() == "start" && a.tags[0].val() == TagValue((uint64_t)a.records[0].len));
        size_t at = 0;
        for (const auto& r : a.records) { CHECK(r.start == at && r.len == 320 + 8 * (first[&r - a.records.data()].size() + 2) + r.stuffed); at += r.len; }
        CHECK(at == a.stream.size());
    }
    std::vector<Float> levels(a.stream);
    levels.insert(levels.end(), b.stream.begin(), b.stream.end());
    for (Float v : levels) if (v != lo && v != hi) { CHECK(!"a level that is neither lo nor hi"); break; }

    // the same bits through the three blocks: HdlcFramer<uint8_t> (FCS only), then Scrambler and NrziEncode as sync blocks of a Graph
    HdlcFramer<uint8_t> plain(RR_FRAME_FCS);
    std::vector<uint8_t> bits = plain.push(first).stream;
    { auto more = plain.push(second).stream; bits.insert(bits.end(), more.begin(), more.end()); }
    CHECK(bits.size() == levels.size());
    {
        auto [src, s0] = VectorSource<uint8_t>::new_(bits);
        auto [scr, s1] = Scrambler::g3ruh(std::move(s0));
        auto [enc, s2] = NrziEncode::new_(std::move(s1));
        CHECK(std::string(scr->block_name()) == "Scrambler" && std::string(enc->block_name()) == "NrziEncode");
        auto sink = std::make_unique<VectorSink<uint8_t>>(std::move(s2));
        auto hook = sink->hook();
        Graph g;
        g.add(std::move(src)); g.add(std::move(scr)); g.add(std::move(enc)); g.add(std::move(sink));
        g.run();
        CHECK(hook->size() == levels.size());
        size_t bad = 0;
        if (hook->size() == levels.size())
            for (size_t i = 0; i < levels.size(); i++) bad += ((*hook)[i] ? hi : lo) != levels[i];
        CHECK(bad == 0);
    }

    // the levels at the bit rate are what the modulator takes (RationalResampler copies samples: the Map commutes with it)
    auto [src, s0] = VectorSource<Float>::new_(levels);
    auto [tx, s1] = FmTx::new_(std::move(s0), interp, deci, k);
    auto sink = std::make_unique<VectorSink<Complex>>(std::move(s1));
    auto hook = sink->hook();
    Graph g;
    g.add(std::move(src)); g.add(std::move(tx)); g.add(std::move(sink));
    g.run();
    CHECK(hook->size() == levels.size() * interp / deci);

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    const uint64_t nl = levels.size(), nc = hook->size();
    std::fwrite(&nl, sizeof nl, 1, o);
    std::fwrite(levels.data(), sizeof(Float), nl, o);
    std::fwrite(&nc, sizeof nc, 1, o);
    for (size_t i = 0; i < nc; i++) { const Complex y = (*hook)[i]; const float re = y.real(), im = y.imag(); std::fwrite(&re, 4, 1, o); std::fwrite(&im, 4, 1, o); }
    std::fclose(o);
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
