// pdu_host.hpp — the host-only logic behind rr_pdu_records, rr_wpcr_process_pdus and rr_wpcr_pack_dev: what is done to records
// once they are in host memory.  No HIP in here, so tests/cpp/test_pdu_hostlogic.cpp builds it with the host sanitizers and
// drives it without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"

namespace rr {

// What rr_stream_to_pdu_create refuses, said before any device is touched; nullptr: fine.
inline const char* pdu_check(size_t max_size, int flags) {
    if (max_size > 512000) return "max_size beyond 512000 samples";
    if (flags & ~RR_PDU_MIDPOINT) return "unknown stream_to_pdu flags";
    return nullptr;
}

// The device appends its records in no order and counts every one it wanted to append: `counted` of them, of which the buffer
// holds at most `held_cap`.  nullptr, or why the count cannot be trusted.
inline const char* pdu_count_check(unsigned long long counted, size_t held_cap) {
    return counted > held_cap ? "stream_to_pdu: record count beyond the window" : nullptr;
}
// ascending; slot[i] = where record i stood in the device's order (what belongs to a record there is found through it)
inline void pdu_sort(std::vector<rr_pdu_record>& r, std::vector<size_t>& slot) {
    slot.resize(r.size());
    for (size_t i = 0; i < slot.size(); i++) slot[i] = i;
    std::sort(slot.begin(), slot.end(), [&](size_t a, size_t b) { return r[a].start < r[b].start; });
    std::vector<rr_pdu_record> sorted(r.size());
    for (size_t i = 0; i < slot.size(); i++) sorted[i] = r[slot[i]];
    r.swap(sorted);
}
// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void pdu_copy_out(const std::vector<rr_pdu_record>& r, rr_pdu_record* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(rr_pdu_record));
}
// The bursts Wpcr gets: the records with ok != 0 (all of them when Midpointer did not run), checked against the geometry
// rr_wpcr_process_dev demands.  nullptr, or what is wrong (nothing may be launched then).
inline const char* pdu_select(const std::vector<rr_pdu_record>& r, bool midpoint, size_t n_total, size_t max_len,
                              std::vector<size_t>& starts, std::vector<size_t>& lens, std::vector<float>& mids) {
    starts.clear(); lens.clear(); mids.clear();
    size_t end = 0;
    for (const rr_pdu_record& p : r) {
        if (p.start < end) return "stream_to_pdu: records overlap";
        if (p.start > n_total || p.len > n_total - p.start) return "stream_to_pdu: record outside the arena";
        if (p.len > max_len) return "stream_to_pdu: record longer than a burst may be";
        end = p.start + p.len;
        if (midpoint && !p.ok) continue;
        starts.push_back(p.start);
        lens.push_back(p.len);
        mids.push_back(midpoint ? p.mid : 0.0f);
    }
    return nullptr;
}

// PduToStream over Wpcr's results: burst b's symbols lie at starts[b] and are res[b].nsyms long.  desc gets one (src, dst, len)
// triple per burst with ok and nsyms > 0, dst running without gaps; returns the symbols in all of them.  nullptr-safe outputs:
// the first min(count, cap) of pdu_start / pdu_len are written.
inline size_t pdu_pack_plan(const std::vector<rr_wpcr_result>& res, const std::vector<size_t>& starts, std::vector<long>& desc,
                            size_t* pdu_start, size_t* pdu_len, size_t cap, size_t* npdus) {
    desc.clear();
    size_t at = 0, k = 0;
    for (size_t b = 0; b < res.size() && b < starts.size(); b++) {
        if (!res[b].ok || res[b].nsyms == 0) continue;
        desc.push_back((long)starts[b]);
        desc.push_back((long)at);
        desc.push_back((long)res[b].nsyms);
        if (k < cap) {
            if (pdu_start) pdu_start[k] = at;
            if (pdu_len) pdu_len[k] = res[b].nsyms;
        }
        at += res[b].nsyms;
        k++;
    }
    if (npdus) *npdus = k;
    return at;
}

}  // namespace rr
