// test_bits_host.cpp — VectorSource<Float> -> BitDecoder -> VectorSink<u8> under the C++ host mirror's Graph
// (rustradio_amd/host/rustradio.hpp).  argv[1] names a file the Python test wrote from tests/bits_model.py:
//   u64 n, f32 x[n], u8 bits[n], u64 ntags, u64 pos[ntags], u8 diffs[ntags]
// the soft symbols and what BinarySlicer -> NrziDecode -> Descrambler::g3ruh -> CorrelateAccessCodeTag(HDLC flag, "sync", 0) make of
// them.  The sink must hold those bits and exactly those tags next to the source's own three.  A second, tiny graph puts a sync
// tag at position 0, where the source's tags sit: they come first (process_sync_tags pushes behind the input's tags).
// Needs a GPU.  Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_bits_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static bool has(const std::vector<Tag>& v, const Tag& t) { return std::find(v.begin(), v.end(), t) != v.end(); }
static long index_of(const std::vector<Tag>& v, const Tag& t) { return (long)(std::find(v.begin(), v.end(), t) - v.begin()); }

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s vectors.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint64_t n = 0, ntags = 0;
    bool ok = fread(&n, 8, 1, f) == 1;
    std::vector<Float> x(n);
    std::vector<uint8_t> bits(n);
    ok = ok && fread(x.data(), 4, n, f) == n && fread(bits.data(), 1, n, f) == n && fread(&ntags, 8, 1, f) == 1;
    std::vector<uint64_t> pos(ntags);
    std::vector<uint8_t> diffs(ntags);
    ok = ok && fread(pos.data(), 8, ntags, f) == ntags && fread(diffs.data(), 1, ntags, f) == ntags;
    fclose(f);
    if (!ok) { printf("short vector file\n"); return 2; }

    const std::vector<uint8_t> flag{0, 1, 1, 1, 1, 1, 1, 0};
    {
        auto [src, s0] = VectorSource<Float>::new_(x);
        auto [dec, s1] = BitDecoder::new_(std::move(s0), RR_BITS_NRZI | RR_BITS_DESCRAMBLE, 0x21, 0, 16, flag, "sync", 0);
        CHECK(std::string(dec->block_name()) == "BitDecoder");
        auto sink = std::make_unique<VectorSink<uint8_t>>(std::move(s1));
        auto hook = sink->hook();
        auto tags = sink->tag_hook();
        Graph g;
        g.add(std::move(src)); g.add(std::move(dec)); g.add(std::move(sink));
        g.run();
        CHECK(*hook == bits);
        CHECK(ntags >= 2 && tags->size() == ntags + 3);
        CHECK(has(*tags, Tag(0, "VectorSource::start", true)));
        CHECK(has(*tags, Tag(0, "VectorSource::first", true)));
        CHECK(has(*tags, Tag(0, "VectorSource::repeat", (uint64_t)0)));
        std::vector<Tag> sync;
        for (auto& t : *tags) if (t.key() == "sync") sync.push_back(t);
        CHECK(sync.size() == ntags);
        for (size_t j = 0; j < ntags && j < sync.size(); j++) CHECK(sync[j] == Tag((size_t)pos[j], "sync", (uint64_t)diffs[j]));
        printf("%zu bits, %zu sync tags\n", hook->size(), sync.size());
    }
    {
        // the slicer alone in front of a one-bit code: +1 matches at 0 and 2; the source's tags at 0 stay ahead of the sync tag at 0
        auto [src, s0] = VectorSource<Float>::new_(std::vector<Float>{1.0f, -1.0f, 1.0f});
        auto [dec, s1] = BitDecoder::new_(std::move(s0), 0, 0, 0, 0, std::vector<uint8_t>{1}, "sync", 0);
        auto sink = std::make_unique<VectorSink<uint8_t>>(std::move(s1));
        auto hook = sink->hook();
        auto tags = sink->tag_hook();
        Graph g;
        g.add(std::move(src)); g.add(std::move(dec)); g.add(std::move(sink));
        g.run();
        CHECK((*hook == std::vector<uint8_t>{1, 0, 1}));
        CHECK(tags->size() == 5);
        const long at0 = index_of(*tags, Tag(0, "sync", (uint64_t)0));
        CHECK(at0 == 3);
        for (const char* k : {"VectorSource::start", "VectorSource::first", "VectorSource::repeat"})
            for (size_t j = 0; j < tags->size(); j++)
                if ((*tags)[j].key() == k) CHECK((long)j < at0 && (*tags)[j].pos() == 0);
        CHECK(tags->size() == 5 && tags->back() == Tag(2, "sync", (uint64_t)0));
    }
    {
        // the separate blocks of the mirror, chained: the same bits
        auto [src, s0] = VectorSource<Float>::new_(x);
        auto [sl, s1] = BinarySlicer::new_(std::move(s0));
        auto [nz, s2] = NrziDecode::new_(std::move(s1));
        auto [ds, s3] = Descrambler::g3ruh(std::move(s2));
        auto [cac, s4] = CorrelateAccessCodeTag::new_(std::move(s3), flag, "sync", 0);
        CHECK(std::string(sl->block_name()) == "BinarySlicer" && std::string(cac->block_name()) == "CorrelateAccessCodeTag");
        auto sink = std::make_unique<VectorSink<uint8_t>>(std::move(s4));
        auto hook = sink->hook();
        auto tags = sink->tag_hook();
        Graph g;
        g.add(std::move(src)); g.add(std::move(sl)); g.add(std::move(nz)); g.add(std::move(ds)); g.add(std::move(cac)); g.add(std::move(sink));
        g.run();
        CHECK(*hook == bits);
        size_t nsync = 0;
        for (auto& t : *tags) if (t.key() == "sync") { CHECK(nsync < ntags && t.pos() == pos[nsync]); nsync++; }
        CHECK(nsync == ntags);
    }
    // a constructor the C ABI refuses throws the library's message
    try {
        auto [src, s0] = VectorSource<uint8_t>::new_(std::vector<uint8_t>{0, 1});
        auto bad = CorrelateAccessCodeTag::new_(std::move(s0), {}, "sync", 0);
        CHECK(false);
    } catch (const Error& e) { CHECK(std::string(e.what()) == "access code must be nonempty"); }
    try {
        auto [src, s0] = VectorSource<uint8_t>::new_(std::vector<uint8_t>{0, 1});
        auto bad = CorrelateAccessCodeTag::new_(std::move(s0), {0, 2, 1}, "sync", 0);
        CHECK(false);
    } catch (const Error& e) { CHECK(std::string(e.what()) == "access code bits must be 0 or 1"); }
    try {
        auto [src, s0] = VectorSource<uint8_t>::new_(std::vector<uint8_t>{0, 1});
        auto bad = Descrambler::new_(std::move(s0), 0x21, 0, 300);
        CHECK(false);
    } catch (const Error& e) { CHECK(std::string(e.what()) == "descrambler length out of range"); }
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
