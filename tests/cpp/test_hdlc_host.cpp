// test_hdlc_host.cpp — the end of the receive chain under the C++ host mirror (rustradio_amd/host/rustradio.hpp): HdlcDeframer in the
// message form of its NCWriteStream<Vec<u8>> output, fed the bits tests/test_gpu_hdlc_host_cpp.py wrote in the windows it names;
// every frame goes back with its packet_pos tag for the test to judge against tests/hdlc_model.py.  On the way packets of its own go
// through HdlcFramer<uint8_t> and come back.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_hdlc_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>
#include <cstring>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

template <class T> static bool rd(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s bits.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint64_t min_size = 0, max_size = 0, keep = 0, fix = 0, nbits = 0, nwin = 0;
    CHECK(rd(f, &min_size) && rd(f, &max_size) && rd(f, &keep) && rd(f, &fix) && rd(f, &nbits) && rd(f, &nwin));
    std::vector<uint8_t> bits(nbits);
    std::vector<uint64_t> win(nwin);
    if (nbits) CHECK(rd(f, bits.data(), nbits));
    if (nwin) CHECK(rd(f, win.data(), nwin));
    std::fclose(f);

    HdlcDeframer d(min_size, max_size, keep != 0, fix != 0);
    const uint64_t M = 8 * max_size + 1;
    CHECK(d.carry_bits() == M + (M - 1) / 5 + 16);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    uint64_t at = 0, total = 0;
    for (uint64_t w : win) {
        CHECK(at + w <= nbits);
        std::vector<bool> repaired;
        auto frames = d.push(std::vector<uint8_t>(bits.begin() + (long)at, bits.begin() + (long)(at + w)), &repaired);
        for (size_t i = 0; i < frames.size(); i++) {
            const auto& [data, tags] = frames[i];
            CHECK(tags.size() == 1 && tags[0].pos() == 0 && tags[0].key() == "packet_pos");
            const uint64_t* pos = std::get_if<uint64_t>(&tags[0].val());
            CHECK(pos && *pos >= at && *pos < at + w);              // the closing flag ended inside this window
            const uint64_t p = pos ? *pos : 0, n = data.size(), r = repaired[i];
            std::fwrite(&p, 8, 1, o); std::fwrite(&n, 8, 1, o); std::fwrite(&r, 8, 1, o);
            if (n) std::fwrite(data.data(), 1, n, o);
            total++;
        }
        at += w;
    }
    const auto s = d.stats();
    const uint64_t end[4] = {~0ull, s.decoded, s.crc_error, s.bitfixed};
    std::fwrite(end, 8, 4, o);
    std::fclose(o);
    CHECK(s.decoded == total);

    // packets of its own through the transmit twin and back: the framer's 20 flags on either side, the FCS checked and stripped
    std::vector<std::vector<uint8_t>> packets;
    for (int k = 0; k < 9; k++) {
        std::vector<uint8_t> p((size_t)(3 + 37 * k));
        for (size_t i = 0; i < p.size(); i++) p[i] = (uint8_t)(k == 4 ? 0xff : 31 * i + 7 * k);
        packets.push_back(p);
    }
    HdlcFramer<uint8_t> fr(RR_FRAME_FCS);
    HdlcDeframer back(1, 400);
    auto got = back.push(fr.push(packets).stream);
    CHECK(got.size() == packets.size());
    for (size_t i = 0; i < got.size() && i < packets.size(); i++) CHECK(got[i].first == packets[i]);
    const auto sb = back.stats();
    CHECK(sb.decoded == packets.size() && sb.crc_error == 0 && sb.bitfixed == 0);
    bool threw = false;
    try { HdlcDeframer bad(1, 65536); } catch (const Error& e) { threw = std::string(e.what()) == "hdlc deframer: max_size beyond 65535"; }
    CHECK(threw);

    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
