// blocks_packet.cpp — host side of the packet-side blocks (blocks_packet.hpp): the sync blocks, the burst and bit blocks, and the
// batch handles (Wpcr, StreamToPdu, Delay, BurstSaver, HdlcFramer, HdlcDeframer, PwmDecoder, SymbolSync, HdlcReceiver, AfskDemod, AmDemod, FskTx, FskTxMulti, KissDecode, KissEncode).  Citations are to the reference's src, as in blocks.cpp.
#include "blocks_packet.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "frame_core.hpp"
#include "frame_host.hpp"
#include "hdlcrx_core.hpp"
#include "kiss_core.hpp"
#include "pdu_host.hpp"
#include "saver_host.hpp"
#include "symsync_host.hpp"
#include "taps.hpp"

namespace rr {

// ---- MultiplyConst, FastFM (sync blocks) ------------------------------------------------------------------------
static int sync_counts(size_t in_len, size_t out_cap, size_t* n, size_t* need) {
    *need = 1;
    if (in_len == 0) { *n = 0; return RR_WAIT_SRC; }
    if (out_cap == 0) { *n = 0; return RR_WAIT_DST; }
    *n = std::min(in_len, out_cap);
    return in_len - *n == 0 ? RR_WAIT_SRC : RR_WAIT_DST;      // the loop's next iteration
}
int SyncBlock::work_dev(const void* in, size_t in_len, void* out, size_t out_cap, size_t* consumed, size_t* produced, size_t* need,
                        hipStream_t s) {
    size_t n = 0;
    const int st = sync_counts(in_len, out_cap, &n, need);
    begin_call();
    if (n) {
        prof_begin(s);
        run(in, out, n, s);
        prof_end(s);
    }
    *consumed = *produced = n;
    return st;
}
MultiplyConst::MultiplyConst(size_t es, float re, float im) : SyncBlock("MultiplyConst", es, es), vr(re), vi(im) {
    if (es != 4 && es != 8) throw Error("MultiplyConst: Float or Complex only");
}
void MultiplyConst::run(const void* in, void* out, size_t n, hipStream_t s) {
    if (in_es == 4) launch_mulconst_f32(static_cast<const float*>(in), static_cast<float*>(out), (long)n, vr, s);
    else launch_mulconst_c32(static_cast<const cf*>(in), static_cast<cf*>(out), (long)n, vr, vi, s);
}
AddConst::AddConst(size_t es, float re, float im) : SyncBlock("AddConst", es, es), vr(re), vi(im) {
    if (es != 4 && es != 8) throw Error("AddConst: Float or Complex only");
}
void AddConst::run(const void* in, void* out, size_t n, hipStream_t s) {
    if (in_es == 4) launch_addconst_f32(static_cast<const float*>(in), static_cast<float*>(out), (long)n, vr, s);
    else launch_addconst_c32(static_cast<const cf*>(in), static_cast<cf*>(out), (long)n, vr, vi, s);
}
FastFM::FastFM() : SyncBlock("FastFM", 8, 4) {
    hist.zero(2, stream);
    RR_HIP(hipStreamSynchronize(stream));
}
void FastFM::run(const void* in, void* out, size_t n, hipStream_t s) {
    VSrc<cf> src{hist.in(), 2, static_cast<const cf*>(in), (long)n};
    launch_fastfm(src, static_cast<float*>(out), (long)n, s);
    launch_vcopy_c32(src, (long)n, hist.out(), 2, s);                // q2, q1 for the next call
    hist.flip();
}

// ---- Vco (vco.rs:9-37) and RationalResampler -> Vco (examples/fm_tx.rs:84-91) ------------------------------------------------
VcoState::VcoState(double kk, hipStream_t s) : k(kk) {
    phase.zero(1, s);                                // phase: 0.0 (vco.rs:18)
    RR_HIP(hipStreamSynchronize(s));
}
Vco::Vco(double k) : SyncBlock("Vco", 4, 8), v(k, stream) {
    zero_copy_in = false;                            // (the scan reads the window twice: tile sums, then the samples)
}
void Vco::run(const void* in, void* out, size_t n, hipStream_t s) {
    launch_vco(static_cast<const float*>(in), static_cast<cf*>(out), (long)n, v.k, v.phase.in(), v.phase.out(), v.scratch(n), s);
    v.phase.flip();
}
FmTx::FmTx(size_t interp, size_t deci, double k) : Resampler("RationalResampler>Vco", interp, deci, 4, 8), v(k, stream) {
    zero_copy_in = false;
}
void FmTx::emit(const void* in, void* out, int64_t r, int64_t n_gather, int64_t c0, hipStream_t s) {
    const int64_t n = r + n_gather;
    if (n <= 0) return;
    launch_fm_tx(static_cast<const float*>(in), static_cast<cf*>(out), (long)r, reinterpret_cast<const float*>(d_pending.p),
                 (long)n_gather, (long)I, (long)D, (long)c0, v.k, v.phase.in(), v.phase.out(), v.scratch((size_t)n), s);
    v.phase.flip();
}

// ---- ComplexToMag2, SinglePoleIirFilter and the burst detector (kernels_burst.hip) ----------------------------------------------
ComplexToMag2::ComplexToMag2() : SyncBlock("ComplexToMag2", 8, 4) {}
void ComplexToMag2::run(const void* in, void* out, size_t n, hipStream_t s) {
    launch_mag2(static_cast<const cf*>(in), static_cast<float*>(out), (long)n, s);
}
AirspyDecode::AirspyDecode() : SyncBlock("AirspyDecode", 4, 8) {}
void AirspyDecode::run(const void* in, void* out, size_t n, hipStream_t s) {
    launch_airspy_decode(static_cast<const unsigned*>(in), static_cast<cf*>(out), (long)n, s);
}
IirState::IirState(float alpha, int nrows, hipStream_t s) : rows(nrows) {
    if (!(alpha >= 0.0f && alpha <= 1.0f)) throw Error("alpha out of range");          // single_pole_iir_filter.rs:38-41 (None)
    const float one_minus = 1.0f - alpha;                                              // :42-43: the reference's two f32 fields
    c.a = (double)alpha;
    c.b = (double)one_minus;
    std::vector<double> p8(IIR_PW8_N), ps(IIR_PWS_N);
    for (int k = 0; k < IIR_PW8_N; k++) p8[k] = (double)powl((long double)c.b, (long double)(8L * k));
    for (int k = 0; k < IIR_PWS_N; k++) ps[k] = (double)powl((long double)c.b, (long double)((long)IIR_SSPAN * k));
    c.bT = p8[IIR_PW8_N - 1];
    pw8.upload(p8.data(), p8.size(), s);
    pws.upload(ps.data(), ps.size(), s);
    c.pw8 = pw8.p;
    c.pws = pws.p;
    y.zero(rows, s);                                 // prev_output: 0 (:25)
    RR_HIP(hipStreamSynchronize(s));
}
SinglePoleIir::SinglePoleIir(float alpha, size_t es)
    : SyncBlock("SinglePoleIirFilter", es == 4 || es == 8 ? es : throw Error("SinglePoleIirFilter: Float or Complex only"), es),
      st(alpha, es == 8 ? 2 : 1, stream) {
    zero_copy_in = false;                            // (the scan reads the window twice: tile responses, then the samples)
}
void SinglePoleIir::run(const void* in, void* out, size_t n, hipStream_t s) {
    if (in_es == 4)
        launch_iir_f32(static_cast<const float*>(in), static_cast<float*>(out), (long)n, st.c, st.y.in(), st.y.out(), st.scratch(n), s);
    else
        launch_iir_c32(static_cast<const cf*>(in), static_cast<cf*>(out), (long)n, st.c, st.y.in(), st.y.out(), st.scratch(n), s);
    st.y.flip();
}
BurstDetector::BurstDetector(float alpha, float threshold)
    : SyncBlock("ComplexToMag2>SinglePoleIirFilter>BurstTagger", 8, 4), st(alpha, 1, stream), thr(threshold) {
    zero_copy_in = false;
    flag.zero(1, stream);                            // last_state: false (burst_tagger.rs:62)
    count.zero(1, stream);
    RR_HIP(hipStreamSynchronize(stream));
}
void BurstDetector::begin_call() {
    edges.clear();
    fetched = true;                                  // a call that moves nothing has no edges and leaves every state alone
}
void BurstDetector::run(const void* in, void* out, size_t n, hipStream_t s) {
    list.reserve(n);
    // (this call's counter was zeroed by the previous call's launch, or at construction; it zeroes the other one)
    launch_burst_detector(static_cast<const cf*>(in), static_cast<float*>(out), (long)n, st.c, st.y.in(), st.y.out(), st.scratch(n), thr,
                          flag.in(), flag.out(), count.out(), count.in(), list.p, s);
    st.y.flip();
    flag.flip();
    count.flip();
    fetched = false;
}
const std::vector<unsigned long long>& BurstDetector::fetch_edges() {
    sync();
    if (!fetched) {
        fetch_counted(count.in(), list.p, list.cap, "burst detector: edge count beyond the window", edges, stream);
        std::sort(edges.begin(), edges.end());       // the device appends in no order; the position is the high part
        fetched = true;
    }
    return edges;
}

// ---- BinarySlicer, NrziDecode, Descrambler, CorrelateAccessCodeTag and their fusion (kernels_bits.hip) ---------------------------
const char* bits_check(int flags, unsigned long long seed, unsigned len, unsigned code_len) {
    if (const char* e = hdlcrx_check_bits(flags, seed, len)) return e;                 // (the stages HdlcReceiver runs as well)
    if (code_len > 64) return "access code longer than 64 bits";
    return nullptr;
}
// RR_BITS_* and Descrambler::new(mask, seed, len) as the stages' configuration (hdlcrx_core.hpp says how the register maps to
// delays) -> the history word in front of the stream: the seed, or 0 without a descrambler
static unsigned long long bits_decode(int flags, unsigned long long mask, unsigned long long seed, unsigned len, BitsCfg& cfg) {
    cfg.invert = flags & RR_BITS_INVERT ? 1 : 0;
    cfg.nrzi = flags & RR_BITS_NRZI ? 1 : 0;
    if (!(flags & RR_BITS_DESCRAMBLE)) return 0;
    cfg.dmask = rx_dmask(mask, len);
    return rx_dhist0(seed, len);
}
BitDecoder::BitDecoder(const char* nm, bool f32src, int flags, unsigned long long mask, unsigned long long seed, unsigned len,
                       unsigned long long code, unsigned code_len, size_t allowed_diffs)
    : SyncBlock(nm, f32src ? 4 : 1, 1) {
    if (const char* e = bits_check(flags, seed, len, code_len)) throw Error(e);
    unsigned long long init[BITS_ST_N] = {0, 0, 0, 0};                                // last: 0 (nrzi.rs:32-33); nothing seen
    init[BITS_ST_DHIST] = bits_decode(flags, mask, seed, len, cfg);
    cfg.L = (int)code_len;
    cfg.code = code_len == 64 ? code : code & ((1ull << code_len) - 1ull);
    cfg.allowed = (unsigned)std::min<size_t>(allowed_diffs, 64);
    st.upload(init, BITS_ST_N, stream);
    total.reserve(1);
    zero_copy_in = false;                            // (tiles re-read their 128 samples of history, and a misaligned window is read one
                                                     //  sample per lane: a page-locked host window is copied down first)
    RR_HIP(hipStreamSynchronize(stream));
}
void BitDecoder::begin_call() {
    tags.clear();
    fetched = true;                                  // a call that moves nothing has no tags and leaves every state alone
}
void BitDecoder::run(const void* in, void* out, size_t n, hipStream_t s) {
    const size_t ntiles = (n + BITS_T - 1) / BITS_T;
    if (cfg.L) { tilecnt.reserve(ntiles); list.reserve(ntiles * BITS_T); }
    if (in_es == 4)
        launch_bits_f32(static_cast<const float*>(in), static_cast<unsigned char*>(out), (long)n, cfg, st.in(), st.out(), tilecnt.p,
                        list.p, s);
    else
        launch_bits_u8(static_cast<const unsigned char*>(in), static_cast<unsigned char*>(out), (long)n, cfg, st.in(), st.out(),
                       tilecnt.p, list.p, s);
    st.flip();
    if (cfg.L) { last_tiles = ntiles; fetched = false; }
}
const std::vector<unsigned long long>& BitDecoder::fetch_tags() {
    sync();
    if (!fetched) {
        // the tiles' entries without the gaps between them, in two small launches; tiles and the entries of a tile are ascending
        offs.reserve(last_tiles);
        launch_bits_tag_offsets(tilecnt.p, (long)last_tiles, offs.p, total.p, stream);
        const auto pack = [&](size_t nt) {
            packed.reserve(nt);
            launch_bits_tag_gather(tilecnt.p, offs.p, list.p, (long)last_tiles, packed.p, stream);
            return packed.p;
        };
        fetch_counted_at(total.p, pack, last_tiles * (size_t)BITS_T, "bit decoder: tag count beyond the window", tags, stream);
        fetched = true;
    }
    return tags;
}

// ---- Wpcr (wpcr.rs:105-239; kernels_wpcr.hip) ---------------------------------------------------------------------------------------
static_assert(sizeof(WpcrResult) == sizeof(rr_wpcr_result) && offsetof(WpcrResult, nsyms) == offsetof(rr_wpcr_result, nsyms) &&
              offsetof(WpcrResult, frequency) == offsetof(rr_wpcr_result, frequency), "WpcrResult is rr_wpcr_result");
Wpcr::Wpcr(float rate)
    : BatchBlock("Wpcr", 4, 4, "Wpcr takes whole bursts: rr_wpcr_process / rr_wpcr_process_dev"), samp_rate(rate) {}
void Wpcr::check(size_t n_total, const size_t* st, const size_t* ln, size_t nbursts) {
    if (nbursts && (!st || !ln)) throw Error("null burst descriptors");
    size_t end = 0;
    for (size_t b = 0; b < nbursts; b++) {
        if (st[b] < end) throw Error("bursts overlap");
        if (st[b] > n_total || ln[b] > n_total - st[b]) throw Error("burst outside the buffer");
        if (ln[b] > MAX_LEN) throw Error("burst longer than 512000 samples");
        end = st[b] + ln[b];
    }
}
void Wpcr::process_dev(const float* d_x, size_t n_total, const size_t* st, const size_t* ln, const float* mid, size_t nbursts,
                       float* d_syms, hipStream_t s) {
    check(n_total, st, ln, nbursts);
    if (nbursts > 0x3fffffff) throw Error("too many bursts");
    starts.assign(st, st + nbursts);
    lens.assign(ln, ln + nbursts);
    results.clear();
    fetched = true;
    if (!nbursts) return;
    // the records, then the burst of every sample tile, then of every bin tile
    size_t nst = 0, nbt = 0;
    for (size_t b = 0; b < nbursts; b++) {
        nst += (ln[b] + WPCR_T - 1) / WPCR_T;
        nbt += ln[b] ? ((ln[b] - 1) / 2 + WPCR_BT - 1) / WPCR_BT : 0;
    }
    if (nst > 0x7fffffff || nbt > 0x7fffffff) throw Error("too many tiles");
    const size_t maps_at = nbursts * sizeof(WpcrBurst), bytes = maps_at + (nst + nbt) * sizeof(int);
    hdesc.resize(bytes);
    WpcrBurst* hb = reinterpret_cast<WpcrBurst*>(hdesc.data());
    int* smap = reinterpret_cast<int*>(hdesc.data() + maps_at);
    int* bmap = smap + nst;
    size_t si = 0, bi = 0;
    for (size_t b = 0; b < nbursts; b++) {
        hb[b].start = (long)st[b];
        hb[b].n = (int)ln[b];
        hb[b].mid = mid ? mid[b] : 0.0f;
        hb[b].stile0 = (int)si;
        hb[b].btile0 = (int)bi;
        const size_t ns = (ln[b] + WPCR_T - 1) / WPCR_T, nb = ln[b] ? ((ln[b] - 1) / 2 + WPCR_BT - 1) / WPCR_BT : 0;
        for (size_t t = 0; t < ns; t++) smap[si++] = (int)b;
        for (size_t t = 0; t < nb; t++) bmap[bi++] = (int)b;
    }
    desc.reserve(bytes);
    list.reserve(n_total);
    mag.reserve(n_total);
    reim.reserve(n_total);
    tilecnt.reserve(std::max<size_t>(nst, 1));
    res.reserve(nbursts);
    hstage().h2d(desc.p, hdesc.data(), bytes, s);                // (through the block's pinned chunks: hdesc is free on return)
    const WpcrBurst* db = reinterpret_cast<const WpcrBurst*>(desc.p);
    const int* dsmap = reinterpret_cast<const int*>(desc.p + maps_at);
    prof_begin(s);
    launch_wpcr(d_x, db, (long)nbursts, dsmap, (long)nst, dsmap + nst, (long)nbt, mid != nullptr, samp_rate, list.p, tilecnt.p, mag.p,
                reim.p, res.p, d_syms, s);
    prof_end(s);
    fetched = false;
}
void Wpcr::process_host(const float* x, size_t n_total, const size_t* st, const size_t* ln, const float* mid, size_t nbursts,
                        float* syms) {
    host_call([&] {
        check(n_total, st, ln, nbursts);
        h_in.reserve(std::max<size_t>(n_total, 1));
        h_out.reserve(std::max<size_t>(n_total, 1));
        // only the span of the bursts crosses the bus, in both directions
        const size_t lo = nbursts ? st[0] : 0, hi = nbursts ? st[nbursts - 1] + ln[nbursts - 1] : 0;
        if (hi > lo) {
            hstage().h2d(h_in.p + lo, x + lo, (hi - lo) * sizeof(float), stream);
            RR_HIP(hipMemsetAsync(h_out.p + lo, 0, (hi - lo) * sizeof(float), stream));
        }
        process_dev(h_in.p, n_total, st, ln, mid, nbursts, h_out.p, stream);
        if (hi > lo) hstage().d2h(syms + lo, h_out.p + lo, (hi - lo) * sizeof(float), stream);
    });
}
const std::vector<WpcrResult>& Wpcr::fetch_results() {
    settle();
    if (!fetched) {
        results.resize(starts.size());
        if (!results.empty()) stage_download_sync(results.data(), res.p, results.size() * sizeof(WpcrResult), stream);
        fetched = true;
    }
    return results;
}
std::vector<float> Wpcr::fetch_spectrum(size_t burst) {
    sync();
    if (burst >= starts.size()) throw Error("rr_debug_wpcr_spectrum: no such burst in the most recent call");
    std::vector<float> m(lens[burst] ? (lens[burst] - 1) / 2 : 0);
    if (!m.empty()) stage_download_sync(m.data(), mag.p + starts[burst], m.size() * sizeof(float), stream);
    return m;
}
void Wpcr::pack_dev(const float* d_syms, float* d_out, size_t out_cap, size_t* produced, size_t* pdu_start, size_t* pdu_len, size_t cap,
                    size_t* npdus, hipStream_t s) {
    const std::vector<WpcrResult>& r = fetch_results();
    std::vector<rr_wpcr_result> res(r.size());
    if (!r.empty()) std::memcpy(res.data(), r.data(), r.size() * sizeof(rr_wpcr_result));
    size_t k = 0;
    const size_t total = pdu_pack_plan(res, starts, hpack, pdu_start, pdu_len, cap, &k);
    if (total > out_cap) throw Error("output shorter than the packed symbols");
    *produced = total;
    *npdus = k;
    if (!total) return;
    if (!d_syms || !d_out) throw Error("rr_wpcr_pack_dev: null argument");
    pack_desc.reserve(hpack.size());
    hstage().h2d(pack_desc.p, hpack.data(), hpack.size() * sizeof(long), s);
    launch_pdu_pack(d_syms, pack_desc.p, (long)(hpack.size() / 3), (long)total, d_out, s);
}

// ---- StreamToPdu (burst_tagger.rs:68-85, stream_to_pdu.rs:198-275, wpcr.rs:62-78; kernels_pdu.hip) -------------------------------------
static_assert(sizeof(PduRec) == sizeof(rr_pdu_record) && offsetof(PduRec, nlow) == offsetof(rr_pdu_record, nlow) &&
              offsetof(PduRec, mid) == offsetof(rr_pdu_record, mid) && offsetof(PduRec, stream_pos) == offsetof(rr_pdu_record, stream_pos),
              "PduRec is rr_pdu_record");
StreamToPdu::StreamToPdu(float threshold, size_t max_sz, size_t tl, int flags, size_t elem)
    : StreamToPdu("BurstTagger>StreamToPdu>Midpointer", "StreamToPdu forms PDUs: rr_stream_to_pdu_push / rr_stream_to_pdu_push_dev",
                  threshold, max_sz, tl, flags, elem) {}
StreamToPdu::StreamToPdu(const char* nm, const char* sentence, float threshold, size_t max_sz, size_t tl, int flags, size_t elem)
    : BatchBlock(nm, elem, elem, sentence),
      thr(threshold), max_size(max_sz),
      tail(std::min(tl, max_sz + 1)),          // (a tail beyond max_size files nothing, like max_size + 1: no sum below overflows)
      midpoint((flags & RR_PDU_MIDPOINT) != 0), es(elem) {
    if (const char* e = pdu_check(max_sz, flags)) throw Error(e);
    if (es != 4 && (es != 8 || midpoint)) throw Error("StreamToPdu: Float, or Complex without Midpointer");
    PduState init{};
    init.free = 0;                             // Unsync, last_state false (stream_to_pdu.rs:102, burst_tagger.rs:62)
    init.open_r = init.open_f = PDU_NONE;
    st.upload(&init, 1, stream);
    etotal.reserve(1);
    count.reserve(1);
    root.reserve(1);
    RR_HIP(hipStreamSynchronize(stream));
}
bool StreamToPdu::begin_push(size_t n) {
    records.clear();
    edgelist.clear();
    fetched = efetched = true;                 // a push that moves nothing has no PDUs and no edges and leaves every state alone
    last_n = n;
    n_total = 0;
    if (!n) return false;
    const size_t ntiles = (n + PDU_T - 1) / PDU_T, nr = n / 2 + 2;
    arena.reserve_out((max_size + n) * (es / 4));
    tilecnt.reserve(ntiles);
    offs.reserve(ntiles);
    edges.reserve(n);
    jmp[0].reserve(nr);
    jmp[1].reserve(nr);
    mark.reserve(nr);
    recs.reserve(nr);
    if (midpoint) ranks.reserve(2 * nr);
    return true;
}
PduArgs StreamToPdu::push_args(const void* d_data, const float* d_trig, size_t n) {
    PduArgs g{};
    g.data = d_data; g.trig = d_trig; g.n = (long)n; g.thr = thr;
    g.max_size = max_size; g.tail = tail; g.w0 = w0; g.C = (long)max_size;
    g.prev_arena = arena.in();                 // (nullptr before the first push: nothing is open then)
    g.n_prev = (long)n_prev;
    g.arena = arena.out();
    g.st_in = st.in(); g.st_out = st.out();
    g.tilecnt = tilecnt.p; g.offs = offs.p; g.etotal = etotal.p; g.edges = edges.p;
    g.jmp0 = jmp[0].p; g.jmp1 = jmp[1].p; g.mark = mark.p; g.root = root.p;
    g.recs = recs.p; g.rec_cap = (long)(n / 2 + 2); g.count = count.p; g.ranks = ranks.p; g.midpoint = midpoint;
    return g;
}
void StreamToPdu::end_push(size_t n) {
    arena.flip();
    st.flip();
    n_prev = n;
    n_total = max_size + n;
    w0 += n;
    fetched = efetched = false;
}
void StreamToPdu::push_dev(const void* d_data, const float* d_trig, size_t n, hipStream_t s) {
    if (n > MAX_WINDOW) throw Error("window longer than 1024000 samples");
    if (!begin_push(n)) return;
    const PduArgs g = push_args(d_data, d_trig, n);
    prof_begin(s);
    launch_pdu(g, s, es == 8 ? PDU_C32 : PDU_F32);
    prof_end(s);
    end_push(n);
}
void StreamToPdu::push_host(const void* data, const float* trig, size_t n) {
    host_call([&] {
        if (n > MAX_WINDOW) throw Error("window longer than 1024000 samples");
        if (n) {
            h_data.reserve(n * (es / 4));
            h_trig.reserve(n);
            hstage().h2d(h_data.p, data, n * es, stream);
            hstage().h2d(h_trig.p, trig, n * sizeof(float), stream);
        }
        push_dev(h_data.p, h_trig.p, n, stream);
    });
}
const std::vector<rr_pdu_record>& StreamToPdu::fetch_records() {
    settle();
    if (!fetched) {
        fetch_counted(count.p, recs.p, recs.cap, pdu_count_check((unsigned long long)recs.cap + 1, recs.cap), records, stream);
        pdu_sort(records, slots);              // the device appends in no order
        fetched = true;
    }
    return records;
}
const std::vector<unsigned>& StreamToPdu::fetch_edges() {
    settle();
    if (!efetched) {
        fetch_counted(etotal.p, edges.p, last_n, "stream_to_pdu: edge count beyond the window", edgelist, stream);
        efetched = true;
    }
    return edgelist;
}
void StreamToPdu::fetch_pdu(size_t idx, void* out, size_t cap) {
    const std::vector<rr_pdu_record>& r = fetch_records();
    if (idx >= r.size()) throw Error("rr_pdu_fetch: no such PDU in the most recent push");
    if (r[idx].start > n_total || r[idx].len > n_total - r[idx].start) throw Error("stream_to_pdu: record outside the arena");
    if (const size_t k = std::min(cap, r[idx].len)) stage_download_sync(out, arena.in() + r[idx].start * (es / 4), k * es, stream);
}
void StreamToPdu::fetch_ranks(size_t idx, float* low, float* high) {
    const std::vector<rr_pdu_record>& r = fetch_records();
    if (!midpoint) throw Error("rr_debug_pdu_ranks: the handle runs no Midpointer");
    if (idx >= r.size() || idx >= slots.size()) throw Error("rr_debug_pdu_ranks: no such PDU in the most recent push");
    float lh[2] = {0.0f, 0.0f};
    stage_download_sync(lh, ranks.p + 2 * slots[idx], sizeof lh, stream);
    *low = lh[0];
    *high = lh[1];
}

// ---- Delay (delay.rs:62-111) and the burst saver (examples/burst_saver.rs:111-131; kernels_saver.hip) --------------------------------
Delay::Delay(size_t d, size_t es) : Block("Delay", es, es), delay(d), remaining(d) {
    if (const char* e = delay_check(d, es)) throw Error(e);
}
int Delay::work_dev(const void* in, size_t in_len, void* out, size_t out_cap, size_t* consumed, size_t* produced, size_t* need,
                    hipStream_t s) {
    const DelayStep d = delay_step(remaining, in_len, out_cap);
    if (d.zeros + d.copied) {
        prof_begin(s);
        launch_delay(in, out, (long)d.zeros, (long)d.copied, in_es, s);
        prof_end(s);
    }
    *consumed = d.copied;
    *produced = d.zeros + d.copied;
    *need = 1;
    return d.status;
}
BurstSaver::BurstSaver(float alpha, float threshold, size_t dl, size_t max_sz, size_t tl)
    : StreamToPdu("ComplexToMag2>SinglePoleIirFilter|Delay>BurstTagger>StreamToPdu",
                  "BurstSaver forms PDUs: rr_burst_saver_push / rr_burst_saver_push_dev", threshold, max_sz, tl, 0, 8),
      iir(alpha, 1, stream), delay(dl) {
    if (const char* e = saver_check(alpha, dl, max_sz)) throw Error(e);
    hist.zero(std::max<size_t>(delay, 1), stream);   // Delay fills with T::default() (delay.rs:87)
    RR_HIP(hipStreamSynchronize(stream));
}
void BurstSaver::push_dev(const cf* d_in, size_t n, float* d_env, hipStream_t s) {
    if (const char* e = saver_push_check(d_in, n)) throw Error(e);
    if (!begin_push(n)) return;
    if (!d_env) { env.reserve(n); d_env = env.p; }
    const PduArgs g = push_args(nullptr, d_env, n);
    const SaverPlan pl = saver_plan(n, delay);
    SaverArgs c{};
    c.x = reinterpret_cast<const unsigned long long*>(d_in);
    c.n = (long)n; c.delay = (long)delay; c.from_hist = (long)pl.from_hist; c.shifted = (long)pl.shifted;
    c.hist_in = hist.in(); c.hist_out = hist.out();
    c.arena = static_cast<unsigned long long*>(g.arena); c.C = g.C;
    c.prev_arena = static_cast<const unsigned long long*>(g.prev_arena); c.n_prev = g.n_prev;
    c.st_in = g.st_in; c.w0 = g.w0;
    prof_begin(s);
    launch_mag2_iir(d_in, d_env, (long)n, iir.c, iir.y.in(), iir.y.out(), iir.scratch(n), s);
    launch_saver_copy(c, s);
    launch_pdu(g, s, PDU_NODATA);
    prof_end(s);
    iir.y.flip();
    hist.flip();
    end_push(n);
}
void BurstSaver::push_host(const cf* in, size_t n, float* out_env) {
    host_call([&] {
        if (const char* e = saver_push_check(in, n)) throw Error(e);
        if (n) {
            h_in.reserve(n);
            hstage().h2d(h_in.p, in, n * sizeof(cf), stream);
            if (out_env) h_env.reserve(n);
        }
        push_dev(h_in.p, n, n && out_env ? h_env.p : nullptr, stream);
        if (n && out_env) stage_download_sync(out_env, h_env.p, n * sizeof(float), stream);
    });
}

// ---- Scrambler::g3ruh, NrziEncode and the HDLC framer (descrambler.rs:41-47, nrzi.rs:52-69, hdlc_framer.rs; kernels_frame.hip) ----------
void LineState::init(int m, hipStream_t s) {
    mode = m;
    if (!mode) return;
    std::vector<unsigned> h(LINE_NP * LINE_NS);
    line_build_powers(mode, h.data());
    pw.upload(h.data(), h.size(), s);
    const unsigned zero = 0;                         // Lfsr::g3ruh's seed 0 (descrambler.rs:31), NrziEncode's out 0 (nrzi.rs:59-60)
    st.upload(&zero, 1, s);
}
void LineState::run(const unsigned char* in, void* out, bool out_f32, float lo, float hi, size_t max_n, const unsigned long long* n_dev,
                    hipStream_t s) {
    if (!max_n) return;
    const size_t ntiles = (max_n + LINE_T - 1) / LINE_T;
    LineArgs a{};
    a.in = in; a.out = out; a.out_f32 = out_f32 ? 1 : 0; a.lo = lo; a.hi = hi;
    a.max_n = (long)max_n; a.n_dev = n_dev; a.mode = mode;
    if (mode) {
        z.reserve(ntiles);
        carry.reserve(ntiles);
        a.pw = pw.p; a.st_in = st.in(); a.st_out = st.out(); a.z = z.p; a.carry = carry.p;
    }
    launch_line(a, s);
    if (mode) st.flip();
}
LineCoder::LineCoder(const char* nm, int mode) : SyncBlock(nm, 1, 1) {
    line.init(mode, stream);
    zero_copy_in = false;                            // (a tile is read twice: a page-locked host window is copied down first)
    RR_HIP(hipStreamSynchronize(stream));
}
void LineCoder::run(const void* in, void* out, size_t n, hipStream_t s) {
    line.run(static_cast<const unsigned char*>(in), out, false, 0.0f, 0.0f, n, nullptr, s);
}

static_assert(sizeof(StuffSum) == 4 * sizeof(unsigned), "FrameArgs::sums: four words per tile");
HdlcFramer::HdlcFramer(int fl, float l, float h)
    : BatchBlock("FcsAdder>HdlcFramer>PduToStream", 1, fl & RR_FRAME_SYMBOLS ? 4 : 1,
                 "HdlcFramer takes whole packets: rr_hdlc_framer_push / rr_hdlc_framer_push_dev"),
      flags(fl), lo(l), hi(h) {
    if (const char* e = frame_check_flags(fl)) throw Error(e);
    line.init((fl & RR_FRAME_G3RUH ? LINE_SCR : 0) | (fl & RR_FRAME_NRZI ? LINE_NRZI : 0), stream);
    total.reserve(1);
    RR_HIP(hipStreamSynchronize(stream));
}
void HdlcFramer::push_dev(const unsigned char* d_bytes, size_t n_bytes, const size_t* st, const size_t* ln, size_t npackets, void* d_out,
                          size_t out_cap, hipStream_t s) {
    size_t bnd = 0;
    if (const char* e = frame_check_push(flags, n_bytes, st, ln, npackets, out_cap, &bnd)) throw Error(e);
    if (npackets && !d_out) throw Error("null output");
    if (npackets && n_bytes && !d_bytes) throw Error("null input");
    lens.assign(ln, ln + npackets);
    bound = bnd;
    records.clear();
    produced = 0;
    fetched = true;                                  // a push of no packets has no records and leaves every state alone
    if (!npackets) return;
    FramePlan pl;
    frame_plan(flags, st, ln, npackets, FRAME_CH, pl);
    const bool fcs = (flags & RR_FRAME_FCS) != 0, coded = line.mode != 0 || (flags & RR_FRAME_SYMBOLS) != 0;
    FrameArgs a{};
    a.P = (long)npackets;
    a.nbytes = (long)pl.nbytes;
    a.ntiles = (long)std::max<size_t>(1, (8 * pl.nbytes + FRAME_T - 1) / FRAME_T);
    a.nchunks = (long)pl.nchunks;
    a.fcs = fcs ? 1 : 0;
    desc.reserve(pl.words.size());
    if (fcs) { part.reserve(std::max<size_t>(pl.nchunks, 1)); crc.reserve(npackets); }
    lb.reserve(std::max<size_t>(pl.nbytes, 1));
    sums.reserve(4 * (size_t)a.ntiles);
    tin.reserve(2 * (size_t)a.ntiles);
    cb.reserve(npackets + 1);
    if (coded) pre.reserve(bnd);
    hstage().h2d(desc.p, pl.words.data(), pl.words.size() * sizeof(unsigned long long), s);      // (pl is free on return)
    a.bytes = d_bytes;
    a.starts = desc.p; a.pb = desc.p + npackets; a.cpre = desc.p + 2 * npackets + 1;
    a.part = part.p; a.crc = crc.p; a.lb = lb.p; a.sums = sums.p; a.tin = tin.p; a.cb = cb.p; a.total = total.p;
    a.pre = coded ? pre.p : static_cast<unsigned char*>(d_out);
    a.cap = (long)bnd;
    prof_begin(s);
    launch_frame(a, s);
    if (coded) line.run(pre.p, d_out, (flags & RR_FRAME_SYMBOLS) != 0, lo, hi, bnd, total.p, s);
    prof_end(s);
    fetched = false;
}
void HdlcFramer::push_host(const unsigned char* bytes, size_t n_bytes, const size_t* st, const size_t* ln, size_t npackets, void* out,
                           size_t out_cap, size_t* prod) {
    host_call([&] {
        size_t bnd = 0;
        if (const char* e = frame_check_push(flags, n_bytes, st, ln, npackets, out_cap, &bnd)) throw Error(e);
        *prod = 0;
        if (!npackets) { push_dev(nullptr, n_bytes, st, ln, 0, nullptr, out_cap, stream); return; }
        h_in.reserve(std::max<size_t>(n_bytes, 1));
        h_out.reserve(std::max<size_t>(bnd * out_es, 1));
        if (n_bytes) hstage().h2d(h_in.p, bytes, n_bytes, stream);
        push_dev(h_in.p, n_bytes, st, ln, npackets, h_out.p, bnd, stream);
        fetch_records();                             // waits; `produced` is checked against the bound in there
        if (produced) hstage().d2h(out, h_out.p, produced * out_es, stream);
        *prod = produced;
    });
}
const std::vector<rr_frame_record>& HdlcFramer::fetch_records() {
    settle();
    if (!fetched) {
        const size_t P = lens.size();
        std::vector<unsigned> hcb(P + 1), hcrc(flags & RR_FRAME_FCS ? P : 0);
        unsigned long long tot = 0;
        stage_download_sync(hcb.data(), cb.p, hcb.size() * sizeof(unsigned), stream);
        if (!hcrc.empty()) stage_download_sync(hcrc.data(), crc.p, hcrc.size() * sizeof(unsigned), stream);
        stage_download_sync(&tot, total.p, sizeof tot, stream);
        if (const char* e = frame_records(flags, lens, hcb, hcrc, tot, bound, records, &produced)) throw Error(e);
        fetched = true;
    }
    return records;
}

// ---- HdlcCore: what HdlcDeframer and HdlcReceiver share (hdlc_deframer.rs:80-232; hdlc_body.hpp) -----------------------------------------
void HdlcCore::init(size_t ns, size_t mn, size_t mx, int fl, hipStream_t s) {
    nstreams = ns; min_size = mn; max_size = mx; flags = fl;
    // Unsynced(0xff) (hdlc_deframer.rs:28-32): 8 ones nobody asks about in front of every stream, and every flag is seen whole
    HdlcState init{};
    init.count = HDLC_HALO;
    init.state = HDLC_U;
    const std::vector<HdlcState> all(ns, init);
    st.upload(all.data(), ns, s);
    const size_t cb = ns * hdlc_carry_bits(mx);
    for (auto& b : cbits.buf) { b.reserve(cb); RR_HIP(hipMemsetAsync(b.p, 1, cb, s)); }
    carry = HDLC_HALO;
    etotal.reserve(ns); pstats.reserve(3 * ns); fin.reserve(ns); count.reserve(1);
}
HdlcRxBounds HdlcCore::plan(size_t n, HdlcArgs& a, HdlcRxArgs* rx) {
    last_carry = carry;
    const HdlcPlan p = hdlc_plan(carry, n, max_size);
    const HdlcRxBounds bd = hdlcrx_bounds(nstreams, carry, n);
    const size_t ns = nstreams;                // (a stream's share of each buffer is its pitch)
    raw.reserve(ns * p.nwords); fl.reserve(ns * p.nwords); ab.reserve(ns * p.nwords); sf.reserve(ns * p.nwords);
    tilecnt.reserve(ns * p.ntiles); offs.reserve(ns * p.ntiles);
    ends.reserve(ns * p.ecap); gmap.reserve(ns * p.ecap); pmap.reserve(ns * p.ecap); bmap.reserve(ns * p.nblocks); bstate.reserve(ns * p.nblocks);
    arena.reserve(std::max<size_t>(bd.arena, 1));
    a.cin = cbits.in(); a.cout = cbits.out(); a.st_in = st.in(); a.st_out = st.out();
    a.carry_cap = (long)p.carry_cap;
    a.nv_max = (long)p.one.nv;
    a.ntiles = (long)p.ntiles;
    a.min_size = min_size; a.max_size = max_size;
    a.keep = (flags & RR_HDLC_KEEP_CHECKSUM) != 0; a.fix = (flags & RR_HDLC_FIX_BITS) != 0;
    a.raw = raw.p; a.fl = fl.p; a.ab = ab.p; a.sf = sf.p; a.tilecnt = tilecnt.p; a.offs = offs.p;
    a.etotal = etotal.p; a.count = count.p; a.pstats = pstats.p;
    a.ends = ends.p; a.ends_cap = (long)p.ecap; a.gmap = gmap.p; a.pmap = pmap.p; a.bmap = bmap.p; a.bstate = bstate.p; a.fin = fin.p;
    a.arena = arena.p; a.arena_cap = (long)p.one.arena; a.rec_cap = (long)bd.frames;
    if (rx) {
        rx->p_words = (long)p.nwords; rx->p_tiles = (long)p.ntiles; rx->p_ends = (long)p.ecap; rx->p_blocks = (long)p.nblocks;
        rx->p_carry = (long)p.carry_cap; rx->p_arena = (long)p.one.arena;
    }
    return bd;
}
void HdlcCore::advance(size_t n) {
    st.flip();
    cbits.flip();
    carry = hdlc_next_carry(carry, n, max_size);
    bfetched = false;
}
std::vector<unsigned long long> HdlcCore::fetch_stats(bool before, hipStream_t s) const {
    std::vector<HdlcState> v(nstreams);
    stage_download_sync(v.data(), before ? st.out() : st.in(), nstreams * sizeof(HdlcState), s);
    std::vector<unsigned long long> out(3 * nstreams);
    for (size_t c = 0; c < nstreams; c++) std::copy(v[c].stats, v[c].stats + 3, out.begin() + 3 * c);
    return out;
}
const std::vector<unsigned char>& HdlcCore::fetch_bytes(hipStream_t s) {
    if (!bfetched) {
        bytes.assign(arena_len(), 0);
        if (!bytes.empty()) stage_download_sync(bytes.data(), arena.p, bytes.size(), s);
        bfetched = true;
    }
    return bytes;
}

// ---- HdlcDeframer (hdlc_deframer.rs:80-232; kernels_hdlc.hip): the one-stream case of HdlcCore over a byte per bit ---------------------
static_assert(sizeof(HdlcRec) == sizeof(rr_hdlc_frame) && offsetof(HdlcRec, pos) == offsetof(rr_hdlc_frame, pos) &&
              offsetof(HdlcRec, start) == offsetof(rr_hdlc_frame, start) && offsetof(HdlcRec, len) == offsetof(rr_hdlc_frame, len) &&
              offsetof(HdlcRec, flags) == offsetof(rr_hdlc_frame, flags), "HdlcRec is rr_hdlc_frame");
HdlcDeframer::HdlcDeframer(size_t mn, size_t mx, int fl)
    : BatchBlock("HdlcDeframer", 1, 1, "HdlcDeframer delivers frames: rr_hdlc_deframer_push / rr_hdlc_deframer_push_dev") {
    if (const char* e = hdlc_check_create(mn, mx, fl)) throw Error(e);
    core.init(1, mn, mx, fl, stream);
    RR_HIP(hipStreamSynchronize(stream));
}
void HdlcDeframer::push_dev(const unsigned char* d_bits, size_t n, hipStream_t s) {
    if (const char* e = hdlc_check_push(d_bits, n)) throw Error(e);
    frames.clear();
    fetched = true;                            // a push of no bits has no frames and leaves every state alone
    core.begin(n);
    if (!n) return;
    HdlcArgs a{};
    const HdlcRxBounds bd = core.plan(n, a, nullptr);
    recs.reserve(std::max<size_t>(bd.frames, 1));
    a.bits = d_bits; a.n = (long)n; a.w0 = w0; a.recs = recs.p;
    prof_begin(s);
    if (bd.arena) RR_HIP(hipMemsetAsync(core.arena.p, 0, bd.arena, s));
    launch_hdlc(a, s);
    prof_end(s);
    core.advance(n);
    w0 += n;
    fetched = false;
}
void HdlcDeframer::push_host(const unsigned char* bits, size_t n) {
    host_call([&] {
        if (const char* e = hdlc_check_push(bits, n)) throw Error(e);
        if (n) {
            h_bits.reserve(n);
            hstage().h2d(h_bits.p, bits, n, stream);
        }
        push_dev(h_bits.p, n, stream);
    });
}
const std::vector<rr_hdlc_frame>& HdlcDeframer::fetch_frames() {
    settle();
    if (!fetched) {
        fetched = true;                        // (a refused push has no frames: the refusal is not repeated)
        const HdlcBounds bd = core.bounds().one;
        unsigned long long k = 0;
        stage_download_sync(&k, core.count.p, sizeof k, stream);
        if (const char* e = hdlc_check_count(k, bd)) throw Error(e);
        std::vector<rr_hdlc_frame> r((size_t)k);
        if (k) stage_download_sync(r.data(), recs.p, (size_t)k * sizeof(rr_hdlc_frame), stream);
        const std::vector<unsigned long long> now = core.fetch_stats(false, stream), before = core.fetch_stats(true, stream);
        const unsigned long long at = w0 - core.last_n;      // (w0 has moved behind the push's bits)
        if (const char* e = hdlc_validate(r, bd, core.max_size, at, core.last_n, before.data(), now.data())) throw Error(e);
        frames.swap(r);
    }
    return frames;
}
const std::vector<unsigned char>& HdlcDeframer::fetch_bytes() {
    fetch_frames();                            // (waits; the arena is read only behind a push whose records stood the checks)
    return core.fetch_bytes(stream);
}
void HdlcDeframer::fetch_stats(unsigned long long out[3]) {
    settle();
    const std::vector<unsigned long long> now = core.fetch_stats(false, stream);
    std::copy(now.begin(), now.end(), out);
}

// ---- KissDecode (kiss.rs:96-228; kernels_kiss.hip) --------------------------------------------------------------------------------------
static_assert(sizeof(KissRec) == sizeof(rr_kiss_packet) && offsetof(KissRec, pos) == offsetof(rr_kiss_packet, pos) &&
              offsetof(KissRec, start) == offsetof(rr_kiss_packet, start) && offsetof(KissRec, len) == offsetof(rr_kiss_packet, len) &&
              offsetof(KissRec, in_bytes) == offsetof(rr_kiss_packet, in_bytes) && offsetof(KissRec, port) == offsetof(rr_kiss_packet, port),
              "KissRec is rr_kiss_packet");
static_assert(KISS_TILE == (size_t)KISS_T, "kiss_host.hpp plans in the kernels' tiles");
KissDecode::KissDecode(size_t mx)
    : BatchBlock("KissFrame>KissDecode", 1, 1, "KissDecode delivers packets: rr_kiss_decode_push / rr_kiss_decode_push_dev"), max_len(mx) {
    if (const char* e = kiss_check_create(mx)) throw Error(e);
    KissState init{};
    init.code = KISS_UNSYNC;                   // FrameState::default() (kiss.rs:140-145)
    st.upload(&init, 1, stream);
    for (auto& b : cbytes.buf) b.reserve(mx);
    count.reserve(2);
    root.reserve(6);
    RR_HIP(hipStreamSynchronize(stream));
}
void KissDecode::push_dev(const unsigned char* d_bytes, size_t n, hipStream_t s) {
    if (const char* e = kiss_check_push(d_bytes, n)) throw Error(e);
    packets.clear();
    bytes.clear();
    fetched = bfetched = true;                 // a push of no bytes has no packets and leaves every state alone
    last_n = n;
    if (!n) return;
    last_carry = carry;
    const KissPlan p = kiss_plan(carry, n);
    sums.reserve(6 * p.ntiles); tin.reserve(6 * p.ntiles); tsum.reserve(5 * p.ntiles); toff.reserve(2 * p.ntiles); obase.reserve(p.ntiles + 1);
    arena.reserve(p.arena_cap);
    recs.reserve(std::max<size_t>(p.rec_cap, 1));
    KissArgs a{};
    a.bytes = d_bytes; a.n = (long)n; a.cin = cbytes.in(); a.cout = cbytes.out(); a.st_in = st.in(); a.st_out = st.out();
    a.max_len = (unsigned)max_len; a.nv_max = (long)p.nv_max; a.ntiles = (long)p.ntiles; a.w0 = w0;
    a.sums = sums.p; a.tin = tin.p; a.root = root.p; a.tsum = tsum.p; a.toff = toff.p; a.obase = obase.p;
    a.arena = arena.p; a.arena_cap = (long)p.arena_cap; a.recs = recs.p; a.rec_cap = (long)p.rec_cap; a.count = count.p;
    prof_begin(s);
    RR_HIP(hipMemsetAsync(obase.p, 0xff, (p.ntiles + 1) * sizeof(unsigned), s));
    launch_kiss_decode(a, s);
    prof_end(s);
    st.flip();
    cbytes.flip();
    carry = kiss_next_carry(carry, n, max_len);
    w0 += n;
    fetched = bfetched = false;
}
void KissDecode::push_host(const unsigned char* hb, size_t n) {
    host_call([&] {
        if (const char* e = kiss_check_push(hb, n)) throw Error(e);
        if (n) {
            h_bytes.reserve(n);
            hstage().h2d(h_bytes.p, hb, n, stream);
        }
        push_dev(h_bytes.p, n, stream);
    });
}
const std::vector<rr_kiss_packet>& KissDecode::fetch_packets() {
    settle();
    if (!fetched) {
        fetched = true;                        // (a refused push has no packets: the refusal is not repeated)
        bfetched = true;
        const KissPlan p = kiss_plan(last_carry, last_n);
        unsigned long long k[2] = {0, 0};
        stage_download_sync(k, count.p, sizeof k, stream);
        if (const char* e = kiss_check_count(k, p)) throw Error(e);
        std::vector<rr_kiss_packet> r((size_t)k[0]);
        if (k[0]) stage_download_sync(r.data(), recs.p, (size_t)k[0] * sizeof(rr_kiss_packet), stream);
        KissState now{}, before{};
        stage_download_sync(&now, st.in(), sizeof now, stream);
        stage_download_sync(&before, st.out(), sizeof before, stream);
        if (const char* e = kiss_validate(r, p, max_len, w0 - last_n, last_n, last_carry, k[1], before.stats, now.stats)) throw Error(e);
        packets.swap(r);
        bytes.assign((size_t)k[1], 0);         // the arena is read only behind a push whose records stood the checks
        bfetched = k[1] == 0;
    }
    return packets;
}
const std::vector<unsigned char>& KissDecode::fetch_bytes() {
    fetch_packets();
    if (!bfetched) {
        stage_download_sync(bytes.data(), arena.p, bytes.size(), stream);
        bfetched = true;
    }
    return bytes;
}
void KissDecode::fetch_stats(unsigned long long out[5]) {
    settle();
    KissState now{};
    stage_download_sync(&now, st.in(), sizeof now, stream);
    std::copy(now.stats, now.stats + 5, out);
}

// ---- KissEncode (kiss.rs:247-286; kernels_kiss.hip) -------------------------------------------------------------------------------------
KissEncode::KissEncode()
    : BatchBlock("KissEncode>PduToStream", 1, 1, "KissEncode takes whole packets: rr_kiss_encode_push / rr_kiss_encode_push_dev") {
    total.reserve(1);
}
void KissEncode::push_dev(const unsigned char* d_bytes, size_t n_bytes, const size_t* st, const size_t* ln, const unsigned* po,
                          size_t npackets, void* d_out, size_t out_cap, hipStream_t s) {
    size_t bnd = 0;
    if (const char* e = kiss_encode_check_push(n_bytes, st, ln, npackets, out_cap, &bnd)) throw Error(e);
    if (npackets && (!d_out || (n_bytes && !d_bytes))) throw Error("kiss encode: null argument");
    lens.assign(ln, ln + npackets);
    if (po) ports.assign(po, po + npackets); else ports.assign(npackets, 0u);
    bound = bnd;
    records.clear();
    produced = 0;
    fetched = true;                            // a push of no packets has no records
    if (!npackets) return;
    KissEncPlan pl;
    kiss_encode_plan(st, ln, po, npackets, pl);
    KissEncArgs a{};
    a.P = (long)npackets;
    a.nbytes = (long)pl.nbytes;
    a.ntiles = (long)std::max<size_t>(1, (pl.nbytes + KISS_T - 1) / KISS_T);
    desc.reserve(pl.words.size());
    tcnt.reserve((size_t)a.ntiles); tin.reserve((size_t)a.ntiles); cb.reserve(npackets + 1);
    hstage().h2d(desc.p, pl.words.data(), pl.words.size() * sizeof(unsigned long long), s);      // (pl is free on return)
    a.bytes = d_bytes;
    a.starts = desc.p; a.pb = desc.p + npackets; a.ports = desc.p + 2 * npackets + 1;
    a.tcnt = tcnt.p; a.tin = tin.p; a.cb = cb.p; a.total = total.p;
    a.out = static_cast<unsigned char*>(d_out);
    a.cap = (long)bnd;
    prof_begin(s);
    launch_kiss_encode(a, s);
    prof_end(s);
    fetched = false;
}
void KissEncode::push_host(const unsigned char* hb, size_t n_bytes, const size_t* st, const size_t* ln, const unsigned* po, size_t npackets,
                           unsigned char* out, size_t out_cap, size_t* prod) {
    host_call([&] {
        size_t bnd = 0;
        if (const char* e = kiss_encode_check_push(n_bytes, st, ln, npackets, out_cap, &bnd)) throw Error(e);
        *prod = 0;
        if (!npackets) { push_dev(nullptr, n_bytes, st, ln, po, 0, nullptr, out_cap, stream); return; }
        h_in.reserve(std::max<size_t>(n_bytes, 1));
        h_out.reserve(std::max<size_t>(bnd, 1));
        if (n_bytes) hstage().h2d(h_in.p, hb, n_bytes, stream);
        push_dev(h_in.p, n_bytes, st, ln, po, npackets, h_out.p, bnd, stream);
        fetch_records();                       // waits; `produced` is checked against the bound in there
        if (produced) hstage().d2h(out, h_out.p, produced, stream);
        *prod = produced;
    });
}
const std::vector<rr_kiss_frame_record>& KissEncode::fetch_records() {
    settle();
    if (!fetched) {
        fetched = true;
        std::vector<unsigned> hcb(lens.size() + 1);
        unsigned long long tot = 0;
        stage_download_sync(hcb.data(), cb.p, hcb.size() * sizeof(unsigned), stream);
        stage_download_sync(&tot, total.p, sizeof tot, stream);
        if (const char* e = kiss_encode_records(lens, ports, hcb, tot, bound, records, &produced)) throw Error(e);
    }
    return records;
}

// ---- PwmDecoder (pwm_decoder.rs:385-513; kernels_pwm.hip) -------------------------------------------------------------------------------
PwmDecoder::PwmDecoder(const PwmCfg& c, size_t es)
    : BatchBlock(es == 8 ? "ComplexToMag2>PwmDecoder" : "PwmDecoder", es, 1,
                 "PwmDecoder delivers frames: rr_pwm_decoder_push / rr_pwm_decoder_push_dev"),
      cfg(c), pitch((size_t)pwm_pitch(c.max_bits)) {
    st.zero(1, stream);                        // low, no run, no pulse, no frame, no candidates at sample 0 (:365-382)
    fbits.zero(pitch, stream);
    cand.zero(pitch * cfg.max_distinct, stream);
    meta.zero(cfg.max_distinct, stream);
    etotal.reserve(1);
    count.reserve(2);
    RR_HIP(hipStreamSynchronize(stream));
}
void PwmDecoder::run(const void* d_samples, size_t n, bool eof, hipStream_t s) {
    last = pwm_plan(n, cfg.max_bits, cfg.max_distinct);
    cls.reserve(std::max<size_t>(last.nthreads, 1)); ebits.reserve(std::max<size_t>(last.nthreads, 1));
    tmap.reserve(std::max<size_t>(last.ntiles, 1)); tstate.reserve(std::max<size_t>(last.ntiles, 1));
    tilecnt.reserve(std::max<size_t>(last.ntiles, 1)); offs.reserve(std::max<size_t>(last.ntiles, 1));
    edges.reserve(std::max<size_t>(last.ecap, 1));
    recs.reserve(last.frames);
    arena.reserve(last.arena);
    PwmArgs a{};
    a.in = d_samples; a.es = (int)in_es; a.eof = eof ? 1 : 0;
    a.n = (long)n; a.ntiles = (long)last.ntiles; a.ecap = (long)last.ecap;
    a.cfg = cfg; a.pitch = pitch;
    a.st_in = st.in(); a.st_out = st.out();
    a.fbits_in = fbits.in(); a.fbits_out = fbits.out();
    a.meta_in = meta.in(); a.meta_out = meta.out();
    a.cand_in = cand.in(); a.cand_out = cand.out();
    a.cls = cls.p; a.tmap = tmap.p; a.tstate = tstate.p; a.ebits = ebits.p;
    a.tilecnt = tilecnt.p; a.offs = offs.p; a.edges = edges.p; a.etotal = etotal.p;
    a.recs = recs.p; a.rec_cap = (long)last.frames; a.arena = arena.p; a.arena_cap = (long)last.arena; a.count = count.p;
    prof_begin(s);
    launch_pwm(a, s);
    prof_end(s);
    st.flip(); fbits.flip(); meta.flip(); cand.flip();
    w0 += n;
    fetched = false;
}
void PwmDecoder::push_dev(const void* d_samples, size_t n, hipStream_t s) {
    if (const char* e = pwm_check_push(d_samples, n, flushed)) throw Error(e);
    frames.clear();
    bits.clear();
    fetched = true;                            // a push of no samples has no frames and leaves every state alone
    last = PwmPlan{};
    if (!n) return;
    run(d_samples, n, false, s);
}
void PwmDecoder::push_host(const void* samples, size_t n) {
    host_call([&] {
        if (const char* e = pwm_check_push(samples, n, flushed)) throw Error(e);
        if (n) {
            h_in.reserve(n * in_es);
            hstage().h2d(h_in.p, samples, n * in_es, stream);
        }
        push_dev(h_in.p, n, stream);
    });
}
void PwmDecoder::flush(hipStream_t s) {
    if (const char* e = pwm_check_push(nullptr, 0, flushed)) throw Error(e);
    frames.clear();
    bits.clear();
    flushed = true;
    run(nullptr, 0, true, s);
}
const std::vector<rr_pwm_frame>& PwmDecoder::fetch_frames() {
    settle();
    if (!fetched) {
        fetched = true;                        // (a refused push has no frames: the refusal is not repeated)
        unsigned long long k[2] = {0, 0};
        stage_download_sync(k, count.p, sizeof k, stream);
        if (const char* e = pwm_check_counts(k[0], k[1], last)) throw Error(e);
        std::vector<rr_pwm_frame> r((size_t)k[0]);
        if (k[0]) stage_download_sync(r.data(), recs.p, (size_t)k[0] * sizeof(rr_pwm_frame), stream);
        if (const char* e = pwm_validate(r, k[1], last, cfg.max_bits, cfg.min_repeats, w0)) throw Error(e);
        std::vector<unsigned char> b((size_t)k[1]);
        if (k[1]) stage_download_sync(b.data(), arena.p, (size_t)k[1], stream);
        if (const char* e = pwm_validate_bits(b)) throw Error(e);
        frames.swap(r);
        bits.swap(b);
    }
    return frames;
}
const std::vector<unsigned char>& PwmDecoder::fetch_bits() {
    fetch_frames();
    return bits;
}

// ---- SymbolSync (symbol_sync.rs:46-217; kernels_sync.hip) ---------------------------------------------------------------------------------
// The mapping of streams to lanes of the clock kernel is a measured choice (profiles/symsync_probe.md): one stream per wave ran a
// stream at 5.1 to 6.8 Msample/s, 64 per wave at 1.6 to 1.9 (nearly every iteration some lane takes the sign-change branch and all
// 64 pay), and up to the 4096 streams a handle takes the device has a SIMD's share for every wave of the first mapping (4096 x
// 16,384: 3.4 ms against 10.5 ms).  So it is one stream per wave at every stream count; rr_build_opts.sync_lanes forces either.
SymbolSync::SymbolSync(float sps, float max_deviation, const float* taps, size_t ntaps, size_t ns)
    : BatchBlock("SymbolSync", 4, 4, "SymbolSync runs nstreams streams: rr_symbol_sync_push / rr_symbol_sync_push_dev"), nstreams(ns) {
    if (const char* e = symsync_check(sps, max_deviation, taps, ntaps, ns)) throw Error(e);
    prm = symsync_params(sps, max_deviation, taps, ntaps);
    const int forced = build_opts().sync_lanes;
    if (forced != 0 && forced != 1 && forced != 64) throw Error("rr_build_opts.sync_lanes: 0, 1 or 64");
    spw = forced ? forced : 1;
    prof_launch = build_opts().sync_prof_launch;
    if (prof_launch < 0 || prof_launch > 3) throw Error("rr_build_opts.sync_prof_launch: 0 .. 3");
    SyncState init{};
    sync_init(init, prm);
    const std::vector<SyncState> all(ns, init);
    st.upload(all.data(), ns, stream);
    count.reserve(ns);
    RR_HIP(hipMemsetAsync(count.p, 0, ns * sizeof(unsigned long long), stream));
    RR_HIP(hipStreamSynchronize(stream));
}
void SymbolSync::push_dev(const float* d_in, size_t in_stride, size_t n, float* d_syms, float* d_clock, size_t out_stride, hipStream_t s) {
    if (const char* e = symsync_check_push(d_in, in_stride, n, d_syms, out_stride)) throw Error(e);
    counts.assign(nstreams, 0);
    last_n = n;
    if (!n) {                                  // a push of no samples produces nothing and leaves every state alone
        RR_HIP(hipMemsetAsync(count.p, 0, nstreams * sizeof(unsigned long long), s));
        fetched = true;
        return;
    }
    SyncArgs a{};
    a.in = d_in; a.in_stride = (long)in_stride; a.n = (long)n; a.nstreams = (long)nstreams;
    a.syms = d_syms; a.clk = d_clock; a.out_stride = (long)out_stride;
    a.nwords = (long)symsync_words(n);
    words.reserve(nstreams * (size_t)a.nwords);
    idx.reserve(nstreams * n);
    a.words = words.p; a.idx = idx.p; a.count = count.p;
    a.st_in = st.in(); a.st_out = st.out();
    a.prm = prm;
    a.spw = spw;
    if (!prof_launch) prof_begin(s);
    for (int k = 1; k <= 3; k++) {
        if (prof_launch == k) prof_begin(s);
        launch_sync(a, k, s);
        if (prof_launch == k) prof_end(s);
    }
    if (!prof_launch) prof_end(s);
    st.flip();
    fetched = false;
}
void SymbolSync::push_host(const float* in, size_t in_stride, size_t n, float* syms, float* clock, size_t out_stride, size_t* produced) {
    host_call([&] {
        if (const char* e = symsync_check_push(in, in_stride, n, syms, out_stride)) throw Error(e);
        if (n) {
            const size_t span = symsync_span(nstreams, in_stride, n);
            h_in.reserve(span);
            h_syms.reserve(nstreams * n);
            if (clock) h_clk.reserve(nstreams * n);
            hstage().h2d(h_in.p, in, span * sizeof(float), stream);
        }
        push_dev(h_in.p, in_stride, n, h_syms.p, clock ? h_clk.p : nullptr, n, stream);
        const std::vector<size_t>& k = fetch_counts();       // waits; clamped to n
        for (size_t c = 0; c < nstreams; c++) {
            if (k[c]) hstage().d2h(syms + c * out_stride, h_syms.p + c * n, k[c] * sizeof(float), stream);
            if (k[c] && clock) hstage().d2h(clock + c * out_stride, h_clk.p + c * n, k[c] * sizeof(float), stream);
            produced[c] = k[c];
        }
    });
}
const std::vector<size_t>& SymbolSync::fetch_counts() {
    settle();
    if (!fetched) {
        std::vector<unsigned long long> raw(nstreams);
        stage_download_sync(raw.data(), count.p, nstreams * sizeof(unsigned long long), stream);
        symsync_clamp_counts(raw.data(), nstreams, last_n, counts);
        fetched = true;
    }
    return counts;
}
SyncState SymbolSync::fetch_state(size_t c) {
    if (c >= nstreams) throw Error("symbol sync: no such stream");
    settle();
    SyncState s{};
    stage_download_sync(&s, st.in() + c, sizeof s, stream);
    return s;
}

// ---- HdlcReceiver (binary_slicer.rs, nrzi.rs, descrambler.rs, hdlc_deframer.rs; kernels_hdlcrx.hip): HdlcCore behind the bit chain ------
static_assert(sizeof(HdlcRxRec) == sizeof(rr_hdlc_stream_frame) && offsetof(HdlcRxRec, pos) == offsetof(rr_hdlc_stream_frame, pos) &&
              offsetof(HdlcRxRec, start) == offsetof(rr_hdlc_stream_frame, start) && offsetof(HdlcRxRec, len) == offsetof(rr_hdlc_stream_frame, len) &&
              offsetof(HdlcRxRec, flags) == offsetof(rr_hdlc_stream_frame, flags) && offsetof(HdlcRxRec, stream) == offsetof(rr_hdlc_stream_frame, stream),
              "HdlcRxRec is rr_hdlc_stream_frame");
HdlcReceiver::HdlcReceiver(size_t ns, int bit_flags, unsigned long long mask, unsigned long long seed, unsigned len, size_t mn, size_t mx,
                           int fl)
    : BatchBlock("HdlcReceiver", 4, 1, "HdlcReceiver delivers frames: rr_hdlc_receiver_push / rr_hdlc_receiver_push_dev") {
    if (const char* e = hdlcrx_check_create(ns, bit_flags, seed, len, mn, mx, fl)) throw Error(e);
    unsigned long long one[RX_ST_N] = {0, 0, 0};                      // last: 0 (nrzi.rs:32-33); no symbol taken yet
    one[RX_ST_DHIST] = bits_decode(bit_flags, mask, seed, len, cfg);
    std::vector<unsigned long long> b0(ns * RX_ST_N);
    for (size_t c = 0; c < ns; c++) std::copy(one, one + RX_ST_N, b0.begin() + c * RX_ST_N);
    bst.upload(b0.data(), b0.size(), stream);
    core.init(ns, mn, mx, fl, stream);
    RR_HIP(hipStreamSynchronize(stream));
}
void HdlcReceiver::push_dev(const float* d_syms, size_t stride, size_t n_cap, const unsigned long long* d_counts, hipStream_t s) {
    if (const char* e = hdlcrx_check_push(core.nstreams, d_syms, stride, n_cap)) throw Error(e);
    frames.clear();
    fetched = true;                            // a push of no symbols has no frames and leaves every state alone
    core.begin(n_cap);
    if (!n_cap) return;
    HdlcRxArgs r{};
    const HdlcRxBounds bd = core.plan(n_cap, r.h, &r);
    recs.reserve(std::max<size_t>(bd.frames, 1));
    r.syms = d_syms; r.stride = (long)stride; r.n_cap = (long)n_cap; r.nstreams = (long)core.nstreams; r.counts = d_counts;
    r.invert = cfg.invert; r.nrzi = cfg.nrzi; r.dmask = cfg.dmask;
    r.bst_in = bst.in(); r.bst_out = bst.out();
    r.recs = recs.p;
    prof_begin(s);
    if (bd.arena) RR_HIP(hipMemsetAsync(core.arena.p, 0, bd.arena, s));
    launch_hdlcrx(r, s);
    prof_end(s);
    bst.flip();
    core.advance(n_cap);
    fetched = false;
}
void HdlcReceiver::push_host(const float* syms, size_t stride, size_t n_cap, const size_t* counts) {
    host_call([&] {
        const size_t nstreams = core.nstreams;
        if (const char* e = hdlcrx_check_push(nstreams, syms, stride, n_cap)) throw Error(e);
        if (n_cap) {
            // only what the counts cover is read from the caller's buffer, as on the device
            h_syms.reserve(nstreams * n_cap);
            std::vector<unsigned long long> k(nstreams, n_cap);
            for (size_t c = 0; c < nstreams; c++) {
                if (counts) k[c] = std::min<unsigned long long>(counts[c], n_cap);
                if (k[c]) hstage().h2d(h_syms.p + c * n_cap, syms + c * stride, (size_t)k[c] * sizeof(float), stream);
            }
            if (counts) {
                h_counts.reserve(nstreams);
                hstage().h2d(h_counts.p, k.data(), nstreams * sizeof(unsigned long long), stream);
            }
        }
        push_dev(h_syms.p, n_cap, n_cap, counts ? h_counts.p : nullptr, stream);
    });
}
const std::vector<rr_hdlc_stream_frame>& HdlcReceiver::fetch_frames() {
    settle();
    if (!fetched) {
        fetched = true;                        // (a refused push has no frames: the refusal is not repeated)
        const HdlcRxBounds bd = core.bounds();
        unsigned long long k = 0;
        stage_download_sync(&k, core.count.p, sizeof k, stream);
        if (const char* e = hdlcrx_check_count(k, bd)) throw Error(e);
        std::vector<rr_hdlc_stream_frame> r((size_t)k);
        if (k) stage_download_sync(r.data(), recs.p, (size_t)k * sizeof(rr_hdlc_stream_frame), stream);
        // the pairs' other halves hold what the push started from
        const std::vector<unsigned long long> s1 = core.fetch_stats(false, stream), s0 = core.fetch_stats(true, stream);
        const std::vector<unsigned long long> p1 = positions(bst.in()), p0 = positions(bst.out());
        std::vector<size_t> moved;
        if (const char* e = hdlcrx_clamp_consumed(p0.data(), p1.data(), core.nstreams, core.last_n, moved)) throw Error(e);
        if (const char* e = hdlcrx_validate(r, bd, core.max_size, p0.data(), moved.data(), s0.data(), s1.data())) throw Error(e);
        frames.swap(r);
    }
    return frames;
}
const std::vector<unsigned char>& HdlcReceiver::fetch_bytes() {
    fetch_frames();                            // (waits; the arena is read only behind a push whose records stood the checks)
    return core.fetch_bytes(stream);
}
std::vector<unsigned long long> HdlcReceiver::fetch_stats() {
    settle();
    return core.fetch_stats(false, stream);
}
std::vector<unsigned long long> HdlcReceiver::fetch_consumed() {
    settle();
    return positions(bst.in());
}
std::vector<unsigned long long> HdlcReceiver::positions(const unsigned long long* d_bst) const {
    std::vector<unsigned long long> b(core.nstreams * RX_ST_N), out(core.nstreams);
    stage_download_sync(b.data(), d_bst, b.size() * sizeof(unsigned long long), stream);
    for (size_t c = 0; c < out.size(); c++) out[c] = b[c * RX_ST_N + RX_ST_POS];
    return out;
}

// ---- Il2pReceiver (binary_slicer.rs:17-19, correlate_access_code.rs:93-118, il2p_deframer.rs:172-237, 247-319; kernels_il2p.hip) ----------
Il2pReceiver::Il2pReceiver(size_t ns, int bit_flags, size_t allowed_diffs)
    : BatchBlock("Il2pReceiver", 4, 1, "Il2pReceiver delivers headers: rr_il2p_receiver_push / rr_il2p_receiver_push_dev"),
      nstreams(ns), invert((bit_flags & RR_BITS_INVERT) != 0), allowed(il2p_clamp_allowed(allowed_diffs)) {
    if (const char* e = il2p_check_create(ns, bit_flags)) throw Error(e);
    st.zero(ns * IL2P_ST_N, stream);              // no symbol taken, no bit seen, nothing blocked, no history (il2p_deframer.rs:143-149)
    stats.reserve(2 * ns);
    RR_HIP(hipMemsetAsync(stats.p, 0, 2 * ns * sizeof(unsigned long long), stream));
    count.reserve(1);
    RR_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), stream));
    RR_HIP(hipStreamSynchronize(stream));
}
void Il2pReceiver::push_dev(const float* d_syms, size_t stride, size_t n_cap, const unsigned long long* d_counts, hipStream_t s) {
    if (const char* e = il2p_check_push(nstreams, d_syms, stride, n_cap)) throw Error(e);
    headers.clear();
    fetched = true;                            // a push of no symbols has no headers and leaves every state alone
    last_n = n_cap;
    if (!n_cap) return;
    const Il2pBounds bd = il2p_bounds(nstreams, n_cap);
    bits.reserve(nstreams * bd.words);
    mw.reserve(nstreams * bd.tiles * IL2P_TW);
    maps.reserve(nstreams * bd.tiles * IL2P_MAP_PITCH);
    entry.reserve(nstreams * bd.tiles);
    recs.reserve(std::max<size_t>(bd.headers, 1));
    Il2pArgs a{};
    a.syms = d_syms; a.stride = (long)stride; a.n_cap = (long)n_cap; a.nstreams = (long)nstreams; a.counts = d_counts;
    a.invert = invert; a.allowed = allowed;
    a.st_in = st.in(); a.st_out = st.out();
    a.bits = bits.p; a.mw = mw.p; a.p_words = (long)bd.words; a.ntiles = (long)bd.tiles;
    a.maps = maps.p; a.entry = entry.p;
    a.recs = recs.p; a.rec_cap = (long)bd.headers; a.count = count.p; a.stats = stats.p;
    prof_begin(s);
    RR_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), s));
    launch_il2p(a, s);
    prof_end(s);
    st.flip();
    fetched = false;
}
void Il2pReceiver::push_host(const float* syms, size_t stride, size_t n_cap, const size_t* counts) {
    host_call([&] {
        if (const char* e = il2p_check_push(nstreams, syms, stride, n_cap)) throw Error(e);
        if (n_cap) {
            // only what the counts cover is read from the caller's buffer, as on the device
            h_syms.reserve(nstreams * n_cap);
            std::vector<unsigned long long> k(nstreams, n_cap);
            for (size_t c = 0; c < nstreams; c++) {
                if (counts) k[c] = std::min<unsigned long long>(counts[c], n_cap);
                if (k[c]) hstage().h2d(h_syms.p + c * n_cap, syms + c * stride, (size_t)k[c] * sizeof(float), stream);
            }
            if (counts) {
                h_counts.reserve(nstreams);
                hstage().h2d(h_counts.p, k.data(), nstreams * sizeof(unsigned long long), stream);
            }
        }
        push_dev(h_syms.p, n_cap, n_cap, counts ? h_counts.p : nullptr, stream);
    });
}
const std::vector<rr_il2p_header>& Il2pReceiver::fetch_headers() {
    settle();
    if (!fetched) {
        fetched = true;                        // (a refused push has no headers: the refusal is not repeated)
        const Il2pBounds bd = il2p_bounds(nstreams, last_n);
        unsigned long long k = 0;
        stage_download_sync(&k, count.p, sizeof k, stream);
        if (const char* e = il2p_check_count(k, bd)) throw Error(e);
        std::vector<rr_il2p_header> r((size_t)k);
        if (k) stage_download_sync(r.data(), recs.p, (size_t)k * sizeof(rr_il2p_header), stream);
        // the pair's other half holds what the push started from
        const std::vector<unsigned long long> p1 = positions(st.in()), p0 = positions(st.out());
        std::vector<size_t> moved;
        if (const char* e = il2p_clamp_consumed(p0.data(), p1.data(), nstreams, last_n, moved)) throw Error(e);
        if (const char* e = il2p_validate(r, bd, p0.data(), moved.data())) throw Error(e);
        headers.swap(r);
    }
    return headers;
}
std::vector<unsigned long long> Il2pReceiver::fetch_stats() {
    settle();
    std::vector<unsigned long long> v(2 * nstreams);
    stage_download_sync(v.data(), stats.p, v.size() * sizeof(unsigned long long), stream);
    return v;
}
std::vector<unsigned long long> Il2pReceiver::fetch_consumed() {
    settle();
    return positions(st.in());
}
std::vector<unsigned long long> Il2pReceiver::positions(const unsigned long long* d_st) const {
    std::vector<unsigned long long> b(nstreams * IL2P_ST_N), out(nstreams);
    stage_download_sync(b.data(), d_st, b.size() * sizeof(unsigned long long), stream);
    for (size_t c = 0; c < out.size(); c++) out[c] = b[c * IL2P_ST_N + IL2P_ST_POS];
    return out;
}

// ---- AfskDemod (hilbert.rs:38-61, quadrature_demod.rs:65-109, fft_filter.rs:365-491, add_const.rs:51-68; kernels_afsk.hip) ---------------
AfskDemod::AfskDemod(size_t ns, size_t hilbert_ntaps, int window, float window_parm, float gn, const float* taps, size_t ntaps, float off)
    : BatchBlock("Hilbert>QuadratureDemod>FftFilterFloat>AddConst", 4, 4,
                 "AfskDemod runs nstreams streams: rr_afsk_demod_push / rr_afsk_demod_push_dev"),
      nstreams(ns), gain(gn), offset(off) {
    if (const char* e = afsk_check(ns, hilbert_ntaps, window, window_parm, gn, taps, ntaps, off)) throw Error(e);
    std::vector<float> win, hil;
    if (!make_window(window, window_parm, hilbert_ntaps, win) || !hilbert_taps(win.data(), hilbert_ntaps, hil))
        throw Error("hilbert filter len must be odd and greater than 1");
    g = afsk_geom((int)hilbert_ntaps, (int)ntaps);
    const std::vector<float> hr = afsk_reversed(hil);
    d_hr.upload(hr.data(), hr.size(), stream);
    d_taps.upload(taps, ntaps, stream);
    carry.zero(ns * (size_t)g.C, stream);
    RR_HIP(hipStreamSynchronize(stream));
}
size_t AfskDemod::push_dev(const float* d_in, size_t in_stride, size_t n, float* d_out, size_t out_stride, hipStream_t s) {
    if (const char* e = afsk_check_push(nstreams, d_in, in_stride, n, d_out, out_stride)) throw Error(e);
    if (!n) return 0;                          // a push of no samples launches nothing and leaves every state alone
    AfskArgs a{};
    a.g = g;
    a.in = d_in; a.in_stride = (long)in_stride;
    a.out = d_out; a.out_stride = (long)out_stride;
    a.carry_in = carry.in(); a.carry_out = carry.out();
    a.taps = d_taps.p; a.hr = d_hr.p;
    a.gain = gain; a.offset = offset;
    afsk_plan(a, total, (long)n);
    prof_begin(s);
    launch_afsk(a, (long)nstreams, s);
    prof_end(s);
    carry.flip();
    total += n;
    return (size_t)a.produced;
}
size_t AfskDemod::push_host(const float* in, size_t in_stride, size_t n, float* out, size_t out_stride) {
    size_t produced = 0;
    host_call([&] {
        if (const char* e = afsk_check_push(nstreams, in, in_stride, n, out, out_stride)) throw Error(e);
        if (!n) return;
        const size_t span = afsk_span(nstreams, in_stride, n);
        h_in.reserve(span);
        h_out.reserve(nstreams * n);
        hstage().h2d(h_in.p, in, span * sizeof(float), stream);
        produced = push_dev(h_in.p, in_stride, n, h_out.p, n, stream);
        for (size_t c = 0; c < nstreams && produced; c++)
            hstage().d2h(out + c * out_stride, h_out.p + c * n, produced * sizeof(float), stream);
    });
    return produced;
}

// ---- AmDemod (examples/airspy_am_decode.rs; fft_filter.rs:365-491, rational_resampler.rs:183-198, multiply_const.rs:20-22; kernels_am.hip) ----
AmDemod::AmDemod(size_t ns, const float* taps, size_t ntaps, size_t interp, size_t deci, float sc)
    : BatchBlock("Norm>FftFilterFloat>RationalResampler>MultiplyConst", 8, 4,
                 "AmDemod runs nstreams streams: rr_am_demod_push / rr_am_demod_push_dev"),
      nstreams(ns), scale(sc) {
    if (const char* err = am_check(ns, taps, ntaps, interp, deci, sc)) throw Error(err);
    g = am_geom_of(ntaps, interp, deci);
    int dev = 0, granted = 0;                        // what a workgroup may take of the LDS: asked, not assumed
    RR_HIP(hipGetDevice(&dev));
    RR_HIP(hipDeviceGetAttribute(&granted, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if ((size_t)granted < am_lds_bytes()) throw Error("am demod: the device grants a workgroup less LDS than a tile needs");
    d_taps.upload(taps, ntaps, stream);
    carry.zero(ns * (size_t)g.C + 1, stream);
    RR_HIP(hipStreamSynchronize(stream));
}
size_t AmDemod::push_dev(const cf* d_in, size_t in_stride, size_t n, float* d_out, size_t out_stride, hipStream_t s) {
    size_t produced = 0;
    if (const char* err = am_check_push(nstreams, g, e, d_in, in_stride, n, d_out, out_stride, &produced)) throw Error(err);
    if (!n) return 0;                          // a push of no samples launches nothing and leaves every state alone
    AmArgs a{};
    a.g = g;
    a.in = reinterpret_cast<const float*>(d_in); a.in_stride = (long)in_stride; a.n = (long)n;
    a.out = d_out; a.out_stride = (long)out_stride; a.produced = (long)produced;
    a.carry_in = carry.in(); a.carry_out = carry.out();
    a.taps = d_taps.p;
    a.scale = scale;
    a.e = e;
    prof_begin(s);
    launch_am(a, (long)nstreams, s);
    prof_end(s);
    carry.flip();
    e = am_next_e(e, (long)n, a.produced, g.I, g.D);
    total += n;
    return produced;
}
size_t AmDemod::push_host(const cf* in, size_t in_stride, size_t n, float* out, size_t out_stride) {
    size_t produced = 0;
    host_call([&] {
        size_t k = 0;
        if (const char* err = am_check_push(nstreams, g, e, in, in_stride, n, out, out_stride, &k)) throw Error(err);
        if (!n) return;
        const size_t span = am_span_elems(nstreams, in_stride, n);
        h_in.reserve(span);
        h_out.reserve(nstreams * k + 1);
        hstage().h2d(h_in.p, in, span * sizeof(cf), stream);
        produced = push_dev(h_in.p, in_stride, n, h_out.p, k, stream);
        for (size_t c = 0; c < nstreams && produced; c++)
            hstage().d2h(out + c * out_stride, h_out.p + c * k, produced * sizeof(float), stream);
    });
    return produced;
}

// ---- FskTx (examples/bell202.rs:166-183, g3ruh.rs:256-272; rational_resampler.rs:183-198, vco.rs:9-37; kernels_tx.hip) ------------
FskTx::FskTx(int md, size_t interp1, size_t deci1, float l, float h, double kk1, float g, size_t interp2, size_t deci2, double kk2)
    : BatchBlock(md == FSK_AFSK ? "Resampler>Map>Vco>Re>MultiplyConst>Resampler>Vco" : "Resampler>Map>Vco>MultiplyConst>Resampler", 1, 8,
                 "FskTx takes pushes of line bits: rr_fsk_tx_push / rr_fsk_tx_push_dev"),
      mode(md), lo(l), hi(h), gain(g), k1(kk1), k2(md == FSK_AFSK ? kk2 : 0.0) {
    if (const char* e = fsk_check(md, interp1, deci1, l, h, kk1, g, interp2, deci2, kk2)) throw Error(e);
    r1 = fsk_ratio((long)interp1, (long)deci1);
    r2 = fsk_ratio((long)interp2, (long)deci2);
    phase.zero(2, stream);                           // phase: 0.0 (vco.rs:18), both
    RR_HIP(hipStreamSynchronize(stream));
}
FskPush FskTx::count(size_t n_bits) const {
    static const char some = 0;                      // (only the lengths are asked about)
    FskPush u{};
    if (const char* e = fsk_check_push(mode, pos, r1, r2, &some, n_bits, &some, (size_t)-1, nullptr, 0, &u)) throw Error(e);
    return u;
}
FskPush FskTx::push_dev(const unsigned char* d_bits, size_t n_bits, cf* d_out, size_t out_cap, float* d_audio, size_t audio_cap,
                        hipStream_t s) {
    FskPush u{};
    if (const char* e = fsk_check_push(mode, pos, r1, r2, d_bits, n_bits, d_out, out_cap, d_audio, audio_cap, &u)) throw Error(e);
    if (!n_bits) return u;                           // an empty push launches nothing and leaves every state alone
    if (u.na) {                                      // (bits that make no audio sample move the first resampler only)
        const size_t na = (size_t)u.na, ntiles = (na + FSK_T - 1) / FSK_T;
        FskTxArgs a{};
        a.bits = d_bits;
        a.n = u.n; a.na = u.na; a.no = u.no;
        a.r1 = r1; a.r2 = r2; a.e1 = u.e1; a.e2 = u.e2;
        a.map_dq = ((long)FSK_B * r2.D) / r2.I; a.map_dr = ((long)FSK_B * r2.D) % r2.I;
        a.dhi = k1 * (double)hi; a.dlo = k1 * (double)lo; a.k2 = k2;
        a.gain = gain;
        a.carry_in = phase.in(); a.carry_out = phase.out();
        tilecnt.reserve(ntiles);
        a.tilecnt = tilecnt.p;
        if (mode == FSK_AFSK) {
            tiles2.reserve(ntiles);
            pre2.reserve(na);
            if (!d_audio) audio.reserve(na);
            a.tiles2 = tiles2.p; a.pre2 = pre2.p; a.audio = d_audio ? d_audio : audio.p;
        } else {
            val.reserve(na);
            a.val = val.p;
        }
        a.out = d_out;
        prof_begin(s);
        launch_fsk_tx(a, mode == FSK_AFSK, s);
        prof_end(s);
        phase.flip();
    }
    pos = u.next;
    return u;
}
FskPush FskTx::push_host(const unsigned char* bits, size_t n_bits, cf* out, size_t out_cap, float* audio_out, size_t audio_cap) {
    FskPush u{};
    host_call([&] {
        if (const char* e = fsk_check_push(mode, pos, r1, r2, bits, n_bits, out, out_cap, audio_out, audio_cap, &u)) throw Error(e);
        if (!n_bits) return;
        h_bits.reserve(n_bits);
        h_out.reserve((size_t)u.no);
        if (audio_out) h_audio.reserve((size_t)u.na);
        hstage().h2d(h_bits.p, bits, n_bits, stream);
        u = push_dev(h_bits.p, n_bits, h_out.p, (size_t)u.no, audio_out ? h_audio.p : nullptr, (size_t)u.na, stream);
        if (u.no) hstage().d2h(out, h_out.p, (size_t)u.no * sizeof(cf), stream);
        if (audio_out && u.na) hstage().d2h(audio_out, h_audio.p, (size_t)u.na * sizeof(float), stream);
    });
    return u;
}

// ---- FskTxMulti: FskTx x nstreams, every stream's state and count on the device (kernels_tx.hip) ------------------------
FskTxMulti::FskTxMulti(size_t ns, int md, size_t interp1, size_t deci1, float l, float h, double kk1, float g, size_t interp2, size_t deci2,
                       double kk2)
    : BatchBlock(md == FSK_AFSK ? "Resampler>Map>Vco>Re>MultiplyConst>Resampler>Vco" : "Resampler>Map>Vco>MultiplyConst>Resampler", 1, 8,
                 "FskTxMulti takes pushes of line bits of nstreams streams: rr_fsk_tx_multi_push / rr_fsk_tx_multi_push_dev"),
      nstreams(ns), mode(md), lo(l), hi(h), gain(g), k1(kk1), k2(md == FSK_AFSK ? kk2 : 0.0) {
    if (const char* e = fsk_multi_check(ns, md, interp1, deci1, l, h, kk1, g, interp2, deci2, kk2)) throw Error(e);
    r1 = fsk_ratio((long)interp1, (long)deci1);
    r2 = fsk_ratio((long)interp2, (long)deci2);
    st.zero(ns, stream);                             // every FskPos at the stream's start, both phases 0.0 (vco.rs:18)
    plan.reserve(ns);
    made.reserve(2 * ns);
    RR_HIP(hipMemsetAsync(made.p, 0, 2 * ns * sizeof(unsigned long long), stream));
    counts.assign(2 * ns, 0);
    RR_HIP(hipStreamSynchronize(stream));
}
void FskTxMulti::push_dev(const unsigned char* d_bits, size_t bits_stride, size_t n_cap, const unsigned long long* d_counts, cf* d_out,
                          size_t out_stride, float* d_audio, size_t audio_stride, hipStream_t s) {
    size_t ac = 0, oc = 0;
    if (const char* e = fsk_multi_check_push(mode, nstreams, r1, r2, bits_bound, d_bits, bits_stride, n_cap, d_out, out_stride, d_audio,
                                             audio_stride, &ac, &oc))
        throw Error(e);
    counts.assign(2 * nstreams, 0);
    last_audio_cap = ac; last_out_cap = oc;
    if (!n_cap) {                                    // a push of no bits makes nothing and leaves every state alone
        RR_HIP(hipMemsetAsync(made.p, 0, 2 * nstreams * sizeof(unsigned long long), s));
        fetched = true;
        return;
    }
    const bool afsk = mode == FSK_AFSK;
    FskTxMultiArgs m{};
    m.bits = d_bits; m.bits_stride = (long)bits_stride; m.n_cap = (long)n_cap; m.nstreams = (long)nstreams;
    m.counts = d_counts;
    m.r1 = r1; m.r2 = r2;
    m.map_dq = ((long)FSK_B * r2.D) / r2.I; m.map_dr = ((long)FSK_B * r2.D) % r2.I;
    m.dhi = k1 * (double)hi; m.dlo = k1 * (double)lo; m.k2 = k2;
    m.gain = gain;
    m.st_in = st.in(); m.st_out = st.out();
    m.plan = plan.p; m.made = made.p;
    m.audio_cap = (long)ac; m.out_cap = (long)oc; m.tpitch = (long)((ac + FSK_T - 1) / FSK_T);
    tilecnt.reserve(nstreams * (size_t)m.tpitch);
    m.tilecnt = tilecnt.p;
    if (afsk) {
        tiles2.reserve(nstreams * (size_t)m.tpitch);
        pre2.reserve(nstreams * ac);
        if (!d_audio) audio.reserve(nstreams * ac);
        m.tiles2 = tiles2.p; m.pre2 = pre2.p;
        m.audio = d_audio ? d_audio : audio.p; m.audio_stride = (long)(d_audio ? audio_stride : ac);
    } else {
        val.reserve(nstreams * ac);
        m.val = val.p;
    }
    m.out = d_out; m.out_stride = (long)out_stride;
    prof_begin(s);
    launch_fsk_tx_multi(m, afsk, s);
    prof_end(s);
    st.flip();
    bits_bound += n_cap;
    fetched = false;
}
void FskTxMulti::push_host(const unsigned char* bits, size_t bits_stride, size_t n_cap, const size_t* cnt, cf* out, size_t out_stride,
                           float* audio_out, size_t audio_stride, size_t* n_out, size_t* n_audio) {
    host_call([&] {
        size_t ac = 0, oc = 0;
        if (const char* e = fsk_multi_check_push(mode, nstreams, r1, r2, bits_bound, bits, bits_stride, n_cap, out, out_stride, audio_out,
                                                 audio_stride, &ac, &oc))
            throw Error(e);
        if (n_cap) {
            // only what the counts cover is read from the caller's buffer, as on the device
            h_bits.reserve(nstreams * n_cap);
            h_out.reserve(nstreams * oc);
            if (audio_out) h_audio.reserve(nstreams * ac);
            std::vector<unsigned long long> k(nstreams, n_cap);
            for (size_t c = 0; c < nstreams; c++) {
                if (cnt) k[c] = std::min<unsigned long long>(cnt[c], n_cap);
                if (k[c]) hstage().h2d(h_bits.p + c * n_cap, bits + c * bits_stride, (size_t)k[c], stream);
            }
            if (cnt) {
                h_counts.reserve(nstreams);
                hstage().h2d(h_counts.p, k.data(), nstreams * sizeof(unsigned long long), stream);
            }
        }
        push_dev(h_bits.p, n_cap, n_cap, cnt ? h_counts.p : nullptr, h_out.p, oc, audio_out ? h_audio.p : nullptr, ac, stream);
        const std::vector<unsigned long long>& k = fetch_counts();       // waits; checked against the bound
        for (size_t c = 0; c < nstreams; c++) {
            const size_t na = (size_t)k[c], no = (size_t)k[nstreams + c];
            if (no) hstage().d2h(out + c * out_stride, h_out.p + c * oc, no * sizeof(cf), stream);
            if (audio_out && na) hstage().d2h(audio_out + c * audio_stride, h_audio.p + c * ac, na * sizeof(float), stream);
            if (n_out) n_out[c] = no;
            if (n_audio) n_audio[c] = na;
        }
    });
}
const std::vector<unsigned long long>& FskTxMulti::fetch_counts() {
    settle();
    if (!fetched) {
        fetched = true;                              // (a refused read-back is not repeated: the counts stay 0)
        std::vector<unsigned long long> raw(2 * nstreams);
        stage_download_sync(raw.data(), made.p, raw.size() * sizeof(unsigned long long), stream);
        if (const char* e = fsk_multi_check_counts(raw.data(), nstreams, last_audio_cap, last_out_cap)) throw Error(e);
        counts = raw;
    }
    return counts;
}
std::vector<FskStream> FskTxMulti::fetch_state() {
    settle();
    std::vector<FskStream> all(nstreams);
    stage_download_sync(all.data(), st.in(), all.size() * sizeof(FskStream), stream);
    return all;
}

}  // namespace rr
