// test_il2p_host.cpp — Il2pReceiver of the C++ host mirror (rustradio_amd/host/rustradio.hpp) on the GPU:
// tests/test_gpu_il2p_host_cpp.py writes ragged pushes of symbols, this program runs them and writes the records back for the
// comparison with tests/il2p_model.py.
//   in:   u64 nstreams, invert, allowed_diffs, npushes, then per push and stream u64 count and the f32 symbols
//   out:  per push u64 nrecords and the 64-byte records; then per stream u64 headers, syncs, consumed; u64 tile_bits, carry_bits
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../rustradio_amd/host/rustradio.hpp"

static uint64_t get64(std::ifstream& f) { uint64_t v = 0; f.read(reinterpret_cast<char*>(&v), 8); return v; }
static void put64(std::ofstream& f, uint64_t v) { f.write(reinterpret_cast<const char*>(&v), 8); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const uint64_t ns = get64(in), invert = get64(in), allowed = get64(in), npushes = get64(in);
        rustradio::Il2pReceiver rx(ns, invert != 0, allowed);
        if (rx.nstreams() != ns) { std::printf("nstreams\n"); return 1; }
        std::ofstream out(argv[2], std::ios::binary);
        for (uint64_t i = 0; i < npushes; i++) {
            std::vector<std::vector<float>> rows(ns);
            for (auto& r : rows) {
                r.resize(get64(in));
                in.read(reinterpret_cast<char*>(r.data()), (std::streamsize)(r.size() * sizeof(float)));
            }
            const std::vector<rr_il2p_header> rec = rx.push(rows);
            if (rec.size() != rx.headers().size()) { std::printf("headers() twice\n"); return 1; }
            put64(out, rec.size());
            out.write(reinterpret_cast<const char*>(rec.data()), (std::streamsize)(rec.size() * sizeof(rr_il2p_header)));
        }
        const auto st = rx.stats();
        const auto used = rx.consumed();
        for (uint64_t c = 0; c < ns; c++) { put64(out, st[c].headers); put64(out, st[c].syncs); put64(out, used[c]); }
        const auto d = rx.dims();
        put64(out, d.first);
        put64(out, d.second);
        // the refusals reach the caller as exceptions
        bool threw = false;
        try { rustradio::Il2pReceiver bad(0); } catch (const rustradio::Error&) { threw = true; }
        if (!threw) { std::printf("nstreams 0 accepted\n"); return 1; }
        threw = false;
        try { rx.push({}); } catch (const rustradio::Error&) { threw = ns != 0; }
        if (!threw) { std::printf("a push without rows accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
