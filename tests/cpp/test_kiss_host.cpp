// test_kiss_host.cpp — KissDecode and KissEncode of the C++ host mirror (rustradio_amd/host/rustradio.hpp) on the GPU:
// tests/test_gpu_kiss_host_cpp.py writes the pushes of a KISS stream, this program decodes them, re-encodes what was delivered
// with the ports it was delivered on, and writes everything back for the comparison with tests/kiss_model.py.
//   in:   u64 max_len, u64 npushes, then per push u64 len and the bytes
//   out:  u64 npackets, per packet u64 push, pos, port, in_bytes, len and the bytes; u64 len and the re-encoded stream; the 5 counters
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
        const uint64_t max_len = get64(in), npushes = get64(in);
        rustradio::KissDecode dec(max_len);
        rustradio::KissEncode enc;
        if (dec.carry_bytes() != max_len) { std::printf("carry_bytes\n"); return 1; }
        std::vector<std::vector<uint8_t>> packets;
        std::vector<unsigned> ports;
        std::vector<uint64_t> meta;
        for (uint64_t i = 0; i < npushes; i++) {
            std::vector<uint8_t> x(get64(in));
            in.read(reinterpret_cast<char*>(x.data()), (std::streamsize)x.size());
            std::vector<uint64_t> pos;
            const auto got = dec.push(x, &pos);
            for (size_t k = 0; k < got.size(); k++) {
                const auto& tags = got[k].second;
                if (tags.size() != 3 || tags[0].key() != "KissDecode:port" || tags[1].key() != "KissDecode:input-bytes" ||
                    tags[2].key() != "KissDecode:output-bytes") { std::printf("tags\n"); return 1; }
                const uint64_t port = std::get<uint64_t>(tags[0].val()), inb = std::get<uint64_t>(tags[1].val());
                if (std::get<uint64_t>(tags[2].val()) != got[k].first.size()) { std::printf("output-bytes\n"); return 1; }
                packets.push_back(got[k].first);
                ports.push_back((unsigned)port);
                meta.insert(meta.end(), {i, pos[k], port, inb});
            }
        }
        const auto frames = enc.push(packets, ports);
        size_t at = 0;
        for (size_t p = 0; p < packets.size(); p++) {
            const rr_kiss_frame_record& r = frames.records[p];
            if (r.start != at || r.len != 3 + packets[p].size() + r.escaped || r.port != ports[p]) { std::printf("records\n"); return 1; }
            at += r.len;
        }
        if (at != frames.stream.size() || enc.push({}).stream.size() != 0) { std::printf("produced\n"); return 1; }
        std::ofstream out(argv[2], std::ios::binary);
        put64(out, packets.size());
        for (size_t p = 0; p < packets.size(); p++) {
            for (int q = 0; q < 4; q++) put64(out, meta[4 * p + q]);
            put64(out, packets[p].size());
            out.write(reinterpret_cast<const char*>(packets[p].data()), (std::streamsize)packets[p].size());
        }
        put64(out, frames.stream.size());
        out.write(reinterpret_cast<const char*>(frames.stream.data()), (std::streamsize)frames.stream.size());
        const auto s = dec.stats();
        for (uint64_t v : {s.frames, s.delivered, s.nondata, s.bad_escape, s.overlong}) put64(out, v);
        std::printf("%zu packets\nOK\n", packets.size());
        return 0;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
}
