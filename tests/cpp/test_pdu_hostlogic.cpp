// The host-only logic of rr_pdu_records, rr_wpcr_process_pdus and rr_wpcr_pack_dev (rustradio_amd/csrc/pdu_host.hpp), driven
// without a device: clamping to cap, the sort, the filter by ok, the geometry checks, the pack plan — and many short-lived
// record vectors, the handle churn of a test suite.  Built with -fsanitize=address,undefined and run by tests/test_pdu_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/pdu_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static rr_pdu_record rec(size_t start, size_t len, int ok = 1, float mid = 0.0f) {
    rr_pdu_record r{};
    r.start = start; r.len = len; r.stream_pos = 1000 + start; r.ok = ok; r.mid = mid; r.mean = mid; r.nlow = len / 2;
    return r;
}

int main() {
    using namespace rr;
    // create-time checks
    CHECK(pdu_check(512000, 0) == nullptr && pdu_check(0, RR_PDU_MIDPOINT) == nullptr);
    CHECK(std::string(pdu_check(512001, 0)) == "max_size beyond 512000 samples");
    CHECK(std::string(pdu_check(10, 2)) == "unknown stream_to_pdu flags");
    CHECK(pdu_count_check(5, 5) == nullptr && pdu_count_check(6, 5) != nullptr);

    // sort + copy_out: every cap around the size, NULL with cap 0, an exactly sized destination (an overrun is the sanitizer's)
    for (size_t n = 0; n <= 9; n++) {
        std::vector<rr_pdu_record> r;
        for (size_t k = 0; k < n; k++) r.push_back(rec(((k * 7) % n) * 10, 5));        // a permutation when gcd(7, n) == 1
        const std::vector<rr_pdu_record> raw(r);
        std::vector<size_t> slot;
        pdu_sort(r, slot);
        CHECK(slot.size() == n);
        for (size_t k = 1; k < n; k++) CHECK(r[k - 1].start <= r[k].start);
        for (size_t k = 0; k < n && k < slot.size(); k++) CHECK(slot[k] < n && raw[slot[k]].start == r[k].start);
        for (size_t cap = 0; cap <= n + 2; cap++) {
            std::vector<rr_pdu_record> out(std::min(cap, n));                          // no slack
            size_t total = 99;
            pdu_copy_out(r, out.empty() ? nullptr : out.data(), cap, &total);
            CHECK(total == n);
            for (size_t k = 0; k < out.size(); k++) CHECK(out[k].start == r[k].start && out[k].stream_pos == r[k].stream_pos);
        }
        size_t total = 99;
        pdu_copy_out(r, nullptr, 0, &total);
        CHECK(total == n);
    }

    // select: the filter by ok and the mids
    {
        std::vector<rr_pdu_record> r{rec(0, 4, 1, 0.5f), rec(4, 6, 0, 9.0f), rec(20, 10, 1, -2.0f)};
        std::vector<size_t> st, ln;
        std::vector<float> md;
        CHECK(pdu_select(r, true, 30, 512000, st, ln, md) == nullptr);
        CHECK(st.size() == 2 && st[0] == 0 && st[1] == 20 && ln[0] == 4 && ln[1] == 10 && md[0] == 0.5f && md[1] == -2.0f);
        CHECK(pdu_select(r, false, 30, 512000, st, ln, md) == nullptr);
        CHECK(st.size() == 3 && md[1] == 0.0f);                                        // without Midpointer every record, mid 0
        // geometry
        CHECK(std::string(pdu_select(r, true, 29, 512000, st, ln, md)) == "stream_to_pdu: record outside the arena");
        CHECK(st.size() <= 3);
        CHECK(std::string(pdu_select(r, true, 30, 9, st, ln, md)) == "stream_to_pdu: record longer than a burst may be");
        r[1].start = 3;
        CHECK(std::string(pdu_select(r, true, 30, 512000, st, ln, md)) == "stream_to_pdu: records overlap");
        r[1] = rec(~(size_t)0 - 2, 6);                                                 // start + len wraps
        CHECK(pdu_select(r, false, 30, 512000, st, ln, md) != nullptr);
        std::vector<rr_pdu_record> none;
        CHECK(pdu_select(none, true, 0, 512000, st, ln, md) == nullptr && st.empty() && ln.empty() && md.empty());
    }

    // pack plan: bursts without symbols leave no gap; cap clamps the two arrays, exactly sized
    {
        std::vector<rr_wpcr_result> res(4);
        for (auto& q : res) q = rr_wpcr_result{};
        res[0].ok = 1; res[0].nsyms = 3;
        res[1].ok = 0; res[1].nsyms = 7;
        res[2].ok = 1; res[2].nsyms = 0;
        res[3].ok = 1; res[3].nsyms = 5;
        std::vector<size_t> starts{10, 20, 30, 40};
        for (size_t cap = 0; cap <= 3; cap++) {
            std::vector<size_t> ps(cap), pl(cap);
            std::vector<long> desc;
            size_t k = 99;
            const size_t total = pdu_pack_plan(res, starts, desc, cap ? ps.data() : nullptr, cap ? pl.data() : nullptr, cap, &k);
            CHECK(total == 8 && k == 2 && desc.size() == 6);
            CHECK(desc[0] == 10 && desc[1] == 0 && desc[2] == 3 && desc[3] == 40 && desc[4] == 3 && desc[5] == 5);
            if (cap >= 1) CHECK(ps[0] == 0 && pl[0] == 3);
            if (cap >= 2) CHECK(ps[1] == 3 && pl[1] == 5);
        }
        std::vector<long> desc;
        size_t k = 99;
        CHECK(pdu_pack_plan({}, {}, desc, nullptr, nullptr, 0, &k) == 0 && k == 0 && desc.empty());
    }

    // churn: many record vectors made, sorted, clamped, selected and dropped in quick succession
    {
        unsigned long long seed = 12345;
        auto rnd = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (size_t)(seed >> 33); };
        for (int it = 0; it < 2000; it++) {
            const size_t n = rnd() % 40;
            std::vector<rr_pdu_record> r;
            size_t at = rnd() % 5;
            for (size_t k = 0; k < n; k++) { const size_t len = 1 + rnd() % 9; r.push_back(rec(at, len, (int)(rnd() % 2))); at += len + rnd() % 3; }
            for (size_t k = n; k > 1; k--) std::swap(r[k - 1], r[rnd() % k]);
            std::vector<size_t> slot;
            pdu_sort(r, slot);
            const size_t cap = rnd() % (n + 3);
            std::vector<rr_pdu_record> out(std::min(cap, n));
            size_t total = 0;
            pdu_copy_out(r, out.empty() ? nullptr : out.data(), cap, &total);
            std::vector<size_t> st, ln;
            std::vector<float> md;
            CHECK(pdu_select(r, true, at, 512000, st, ln, md) == nullptr);
            size_t oks = 0;
            for (const auto& q : r) oks += q.ok ? 1 : 0;
            CHECK(total == n && st.size() == oks && ln.size() == oks && md.size() == oks);
        }
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("pdu host logic ok\n");
    return 0;
}
