// abi.cpp — the extern "C" surface declared in include/rustradio_amd.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>

#include "blocks.hpp"
#include "dstream.hpp"
#include "frame_core.hpp"
#include "frame_host.hpp"
#include "hdlc_host.hpp"
#include "hdlcrx_host.hpp"
#include "il2p_host.hpp"
#include "kiss_core.hpp"
#include "kiss_host.hpp"
#include "pdu_host.hpp"
#include "saver_host.hpp"
#include "symsync_host.hpp"
#include "taps.hpp"

struct rr_block {
    std::unique_ptr<rr::Block> b;
    int tag_rule = RR_TAGS_DROP;      // rr_block_tag_rule: what the reference block(s) behind the handle do with tags
    size_t tag_param = 1;
};
// One ring + what makes it a two-ended stream between threads: every entry point takes `m` (two rings: both, deadlock-free),
// produce / consume / close wake `cv`.  closed[side] is the reference's Arc strong count dropping to 1
// (src/stream.rs:148-150,166-168): the shim sets it when it drops its WriteStream / ReadStream end.
struct rr_dstream {
    std::unique_ptr<rr::DStream> s;
    std::mutex m;
    std::condition_variable cv;
    bool closed[2] = {false, false};
    size_t id = 0;
};

namespace rr {
std::atomic<unsigned long long> g_kernel_launches{0};
static thread_local std::string g_err;
void set_last_error(const std::string& m) { g_err = m; }
static thread_local BuildOpts g_opts;
const BuildOpts& build_opts() { return g_opts; }
void set_build_opts(const BuildOpts* o) { g_opts = o ? *o : BuildOpts(); }
// the pending overrides belong to ONE create call: cleared when it returns, whether it succeeded or not
struct OptsScope { ~OptsScope() { set_build_opts(nullptr); } };
}  // namespace rr

template <class F> static rr_block* make_block(F&& f, int tag_rule = RR_TAGS_DROP, size_t tag_param = 1) {
    rr::OptsScope scope;
    try {
        std::unique_ptr<rr::Block> b(f());         // a throwing constructor leaks nothing
        if (const int v = rr::build_opts().host_in_staged) b->zero_copy_in = v < 0;   // (rr_build_opts: the block's default otherwise)
        auto* h = new rr_block;
        h->b = std::move(b);
        h->tag_rule = tag_rule;
        h->tag_param = tag_param;
        return h;
    } catch (const std::exception& e) {
        rr::set_last_error(e.what());
        return nullptr;
    } catch (...) {
        rr::set_last_error("non-standard exception");
        return nullptr;
    }
}

template <class F> static int guarded(F&& f) {
    try { f(); return 0; }
    catch (const std::exception& e) { rr::set_last_error(e.what()); return RR_ERR; } catch (...) { rr::set_last_error("non-standard exception"); return RR_ERR; }
}
// f on the handle's device; with the caller's stream, used as given (see rr_block_work_dev) and what sync() then waits for
template <class B, class F> static int on_device(B* h, F&& f) {
    return guarded([&] { RR_HIP(hipSetDevice(h->device)); f(); });
}
template <class B, class F> static int on_device(B* h, void* hip_stream, F&& f) {
    return on_device(h, [&] { hipStream_t s = static_cast<hipStream_t>(hip_stream); h->last_stream = s; f(s); });
}
// the block of kind T behind a handle, or nullptr and "<what>: <not_a>" (also said when the caller's `args_ok` is false)
template <class T> static T* as(const rr_block* b, const char* what, const char* not_a, bool args_ok = true) {
    auto* p = b && args_ok ? dynamic_cast<T*>(b->b.get()) : nullptr;
    if (!p) rr::set_last_error(std::string(what) + ": " + not_a);
    return p;
}
static const char NOT_WPCR[] = "not a wpcr handle", NOT_PDU[] = "not a stream_to_pdu handle", NOT_FRAMER[] = "not an hdlc framer handle";
static const char NOT_DEFRAMER[] = "not an hdlc deframer handle", NOT_SYNC[] = "not a symbol sync handle", NOT_AFSK[] = "not an afsk demod handle";
static const char NOT_AM[] = "not an am demod handle";
static const char NOT_RECEIVER[] = "not an hdlc receiver handle", NOT_PWM[] = "not a pwm decoder handle";
static const char NOT_IL2P[] = "not an il2p receiver handle";
static const char NOT_FSK[] = "not an fsk tx handle", NOT_FSKM[] = "not an fsk tx multi handle";
static const char NOT_KISSDEC[] = "not a kiss decode handle", NOT_KISSENC[] = "not a kiss encode handle";
// a fetched list of (pos << shift) | val entries into the caller's two arrays
template <class E> static void unpack(const std::vector<E>& e, unsigned shift, size_t* pos, unsigned char* val, size_t cap, size_t* total) {
    *total = e.size();
    for (size_t j = 0; j < e.size() && j < cap; j++) { pos[j] = (size_t)(e[j] >> shift); val[j] = (unsigned char)(e[j] & ((E(1) << shift) - 1)); }
}
// a create call that refuses before any device is touched: it ends the pending overrides like any other (OptsScope)
static rr_block* refuse_create(const char* msg) {
    rr::OptsScope scope;
    rr::set_last_error(msg);
    return nullptr;
}

extern "C" {

int rr_abi_version(void) { return RR_ABI_VERSION; }
int rr_next_create_options(const rr_build_opts* o) {
    if (!o) { rr::set_build_opts(nullptr); return 0; }
    rr::BuildOpts b;
    b.fir_path = o->fir_path; b.fir_prune = o->fir_prune; b.fir_half = o->fir_half; b.fir_cfg = o->fir_cfg_plus1 - 1;
    b.fft_log2f = o->fft_log2f; b.fft_no_split = o->fft_no_split; b.fftfloat_complex = o->fftfloat_complex;
    b.fm_full = o->fm_full; b.fm_poly = o->fm_poly; b.dstream_no_vmm = o->dstream_no_vmm;
    b.fir_poly = o->fir_poly; b.fft_nonfinite_tiles = o->fft_nonfinite_tiles; b.host_in_staged = o->host_in_staged;
    b.sync_lanes = o->sync_lanes; b.sync_prof_launch = o->sync_prof_launch;
    if (b.fir_path < 0 || b.fir_path > 2 || b.fir_cfg > 7 || (b.fft_log2f != 0 && (b.fft_log2f < 10 || b.fft_log2f > 14))) {
        rr::set_last_error("rr_next_create_options: value out of range");
        return RR_ERR;
    }
    rr::set_build_opts(&b);
    return 0;
}
const char* rr_last_error(void) { return rr::g_err.c_str(); }

int rr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int rr_set_device(int ordinal) {
    int n = rr_device_count();
    if (ordinal < 0 || ordinal >= n) { rr::set_last_error("rr_set_device: ordinal out of range"); return RR_ERR; }
    rr::set_thread_device(ordinal);
    return 0;
}

float rr_max_attenuation(int window) { return rr::max_attenuation(window); }
int rr_make_window(int window, float parm, size_t ntaps, float* out) {
    std::vector<float> w;
    if (!rr::make_window(window, parm, ntaps, w)) { rr::set_last_error("unknown window type"); return RR_ERR; }
    if (ntaps) std::memcpy(out, w.data(), ntaps * sizeof(float));
    return 0;
}
size_t rr_compute_ntaps(float samp_rate, float twidth, int window) { return rr::compute_ntaps(samp_rate, twidth, window); }
size_t rr_low_pass(float samp_rate, float cutoff, float twidth, int window, float parm, float* out, size_t cap) {
    std::vector<float> t;
    if (!rr::low_pass(samp_rate, cutoff, twidth, window, parm, t)) {
        rr::set_last_error("low_pass: samp_rate, cutoff and twidth must be > 0 and the window type valid");
        return 0;
    }
    for (size_t i = 0; i < t.size() && i < cap; i++) out[i] = t[i];
    return t.size();
}
size_t rr_low_pass_complex(float samp_rate, float cutoff, float twidth, int window, float parm, rr_c32* out, size_t cap) {
    std::vector<float> t;
    if (!rr::low_pass(samp_rate, cutoff, twidth, window, parm, t)) {
        rr::set_last_error("low_pass_complex: samp_rate, cutoff and twidth must be > 0 and the window type valid");
        return 0;
    }
    for (size_t i = 0; i < t.size() && i < cap; i++) out[i] = rr_c32{t[i], 0.0f};   // fir.rs:602
    return t.size();
}
int rr_multiband(const float* bands, size_t nbands, const float* window, size_t ntaps, rr_c32* out) {
    std::vector<float> t;
    if (!bands && nbands) { rr::set_last_error("multiband: null bands"); return RR_ERR; }
    if (!rr::multiband(bands, nbands, window, ntaps, t)) { rr::set_last_error("multiband: None (fir.rs:558-569)"); return RR_ERR; }
    std::memcpy(out, t.data(), ntaps * sizeof(rr_c32));
    return 0;
}
int rr_hilbert_taps(const float* window, size_t ntaps, float* out) {
    std::vector<float> t;
    if (!rr::hilbert_taps(window, ntaps, t)) { rr::set_last_error("hilbert: window must have more than 1 tap"); return RR_ERR; }
    std::memcpy(out, t.data(), ntaps * sizeof(float));
    return 0;
}

rr_block* rr_fir_c32_create(const rr_c32* taps, size_t ntaps, size_t deci, int translate, float samp_rate, float freq) {
    return make_block([&] { return new rr::FirC32(taps, ntaps, deci, translate != 0, samp_rate, freq); }, RR_TAGS_FORWARD, deci);
}
rr_block* rr_fir_f32_create(const float* taps, size_t ntaps, size_t deci) {
    return make_block([&] { return new rr::FirF32(taps, ntaps, deci); }, RR_TAGS_FORWARD, deci);
}
rr_block* rr_fftfilter_create(const rr_c32* taps, size_t ntaps) {
    return make_block([&] { auto* f = new rr::FftFilter(taps, ntaps); std::unique_ptr<rr::FftFilter> own(f); f->ref_blocks_on(taps); return own.release(); },
                      RR_TAGS_FORWARD, 1);
}
rr_block* rr_fftfilter_float_create(const float* taps, size_t ntaps) {
    return make_block([&] { return new rr::FftFilterFloat(taps, ntaps); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_resampler_create(size_t interp, size_t deci, size_t elem_size) {
    return make_block([&] { return new rr::Resampler(interp, deci, elem_size); });
}
rr_block* rr_fm_chain_u8_create(const rr_c32* taps, size_t ntaps, size_t interp, size_t deci, float gain,
                                int atan2_mode) {
    return make_block([&] { return rr::make_fm_chain(taps, ntaps, interp, deci, gain, atan2_mode, true, nullptr, 0); });
}
rr_block* rr_hilbert_fir_create(size_t hilbert_ntaps, int window, float window_parm, const rr_c32* taps, size_t ntaps,
                                size_t deci, int translate, float samp_rate, float freq) {
    return make_block([&] {
        return new rr::HilbertFir(hilbert_ntaps, window, window_parm, taps, ntaps, deci, translate != 0, samp_rate, freq);
    }, RR_TAGS_FORWARD, deci);
}
rr_block* rr_fftstream_create(size_t size) {
    return make_block([&] { return new rr::FftStream(size); }, RR_TAGS_FRAMES, size);
}
int rr_fft_process(rr_block* b, const rr_c32* msg, size_t n, rr_c32* out) {
    auto* f = b ? dynamic_cast<rr::FftStream*>(b->b.get()) : nullptr;
    if (!f || !msg || !out) { rr::set_last_error("rr_fft_process: not an FftStream handle / null argument"); return RR_ERR; }
    if (n != f->size) {                                                   // fft.rs:46-52
        rr::set_last_error("FFT expected " + std::to_string(f->size) + " samples, got " + std::to_string(n));
        return RR_ERR;
    }
    size_t c = 0, p = 0, need = 0;
    const int st = rr_block_work(b, msg, n, out, n, &c, &p, &need);
    return st == RR_ERR ? RR_ERR : (p == n ? 0 : RR_ERR);
}
rr_block* rr_multiply_const_f32_create(float val) {
    return make_block([&] { return new rr::MultiplyConst(4, val, 0.0f); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_multiply_const_c32_create(float re, float im) {
    return make_block([&] { return new rr::MultiplyConst(8, re, im); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_add_const_f32_create(float val) {
    return make_block([&] { return new rr::AddConst(4, val, 0.0f); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_add_const_c32_create(float re, float im) {
    return make_block([&] { return new rr::AddConst(8, re, im); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_fastfm_create(void) {
    return make_block([&] { return new rr::FastFM(); }, RR_TAGS_FORWARD, 1);
}
static double f64_from_bits(unsigned long long bits) {
    double k;
    static_assert(sizeof k == sizeof bits, "binary64");
    std::memcpy(&k, &bits, sizeof k);
    return k;
}
rr_block* rr_vco_create(unsigned long long k_bits) {
    return make_block([&] { return new rr::Vco(f64_from_bits(k_bits)); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_fm_tx_create(size_t interp, size_t deci, unsigned long long k_bits) {
    return make_block([&] { return new rr::FmTx(interp, deci, f64_from_bits(k_bits)); });
}
rr_block* rr_complex_to_mag2_create(void) {
    return make_block([&] { return new rr::ComplexToMag2(); }, RR_TAGS_FORWARD, 1);
}
// single_pole_iir_filter.rs:38-41: None unless 0 <= alpha <= 1 (NaN fails both comparisons) — said before any device is touched
static bool iir_alpha_ok(float alpha) { return alpha >= 0.0f && alpha <= 1.0f; }
rr_block* rr_single_pole_iir_create(float alpha, size_t elem_size) {
    if (!iir_alpha_ok(alpha)) return refuse_create("alpha out of range");
    return make_block([&] { return new rr::SinglePoleIir(alpha, elem_size); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_burst_detector_create(float alpha, float threshold) {
    if (!iir_alpha_ok(alpha)) return refuse_create("alpha out of range");
    return make_block([&] { return new rr::BurstDetector(alpha, threshold); }, RR_TAGS_FORWARD, 1);
}
int rr_burst_edges(rr_block* b, size_t* pos, unsigned char* val, size_t cap, size_t* total) {
    auto* d = as<rr::BurstDetector>(b, "rr_burst_edges", "not a burst detector handle / null argument", total && (!cap || (pos && val)));
    if (!d) return RR_ERR;
    return on_device(d, [&] { unpack(d->fetch_edges(), 1, pos, val, cap, total); });
}
// the bit-level blocks: parameter errors are said before any device is touched
static rr_block* make_bits(const char* nm, bool f32src, int flags, unsigned long long mask, unsigned long long seed, unsigned len,
                           unsigned long long code, unsigned code_len, size_t allowed_diffs) {
    if (const char* e = rr::bits_check(flags, seed, len, code_len)) return refuse_create(e);
    return make_block([&] { return new rr::BitDecoder(nm, f32src, flags, mask, seed, len, code, code_len, allowed_diffs); },
                      RR_TAGS_FORWARD, 1);
}
rr_block* rr_binary_slicer_create(void) { return make_bits("BinarySlicer", true, 0, 0, 0, 0, 0, 0, 0); }
rr_block* rr_nrzi_decode_create(void) { return make_bits("NrziDecode", false, RR_BITS_NRZI, 0, 0, 0, 0, 0, 0); }
rr_block* rr_descrambler_create(unsigned long long mask, unsigned long long seed, unsigned len) {
    return make_bits("Descrambler", false, RR_BITS_DESCRAMBLE, mask, seed, len, 0, 0, 0);
}
rr_block* rr_correlate_access_code_tag_create(unsigned long long code, unsigned code_len, size_t allowed_diffs) {
    if (code_len == 0) return refuse_create("access code must be nonempty");     // correlate_access_code.rs:79 (assert)
    return make_bits("CorrelateAccessCodeTag", false, 0, 0, 0, 0, code, code_len, allowed_diffs);
}
rr_block* rr_bit_decoder_create(int flags, unsigned long long mask, unsigned long long seed, unsigned len, unsigned long long code,
                                unsigned code_len, size_t allowed_diffs) {
    return make_bits("BitDecoder", true, flags, mask, seed, len, code, code_len, allowed_diffs);
}
int rr_bit_tags(rr_block* b, size_t* pos, unsigned char* diffs, size_t cap, size_t* total) {
    static const char NOT_A[] = "not a handle with a correlator stage / null argument";
    auto* d = as<rr::BitDecoder>(b, "rr_bit_tags", NOT_A, total && (!cap || (pos && diffs)));
    if (d && !d->has_correlator()) d = as<rr::BitDecoder>(nullptr, "rr_bit_tags", NOT_A);
    if (!d) return RR_ERR;
    return on_device(d, [&] { unpack(d->fetch_tags(), 8, pos, diffs, cap, total); });
}
rr_block* rr_wpcr_create(float samp_rate) {
    return make_block([&] { return new rr::Wpcr(samp_rate); });
}
int rr_wpcr_process_dev(rr_block* b, const void* d_samples, size_t n_total, size_t* starts, size_t* lens, const float* mid,
                        size_t nbursts, void* d_syms, void* hip_stream) {
    auto* w = as<rr::Wpcr>(b, "rr_wpcr_process_dev", NOT_WPCR);
    if (!w) return RR_ERR;
    if (nbursts && (!d_samples || !d_syms || !starts || !lens)) { rr::set_last_error("rr_wpcr_process_dev: null argument"); return RR_ERR; }
    return on_device(w, hip_stream, [&](hipStream_t s) {
        w->process_dev(static_cast<const float*>(d_samples), n_total, starts, lens, mid, nbursts, static_cast<float*>(d_syms), s);
    });
}
int rr_wpcr_process(rr_block* b, const float* samples, size_t n_total, size_t* starts, size_t* lens, const float* mid, size_t nbursts,
                    float* syms) {
    auto* w = as<rr::Wpcr>(b, "rr_wpcr_process", NOT_WPCR);
    if (!w) return RR_ERR;
    if (nbursts && (!samples || !syms || !starts || !lens)) { rr::set_last_error("rr_wpcr_process: null argument"); return RR_ERR; }
    return guarded([&] { w->process_host(samples, n_total, starts, lens, mid, nbursts, syms); });
}
int rr_wpcr_results(rr_block* b, rr_wpcr_result* res, size_t cap, size_t* total) {
    auto* w = as<rr::Wpcr>(b, "rr_wpcr_results", NOT_WPCR);
    if (!w) return RR_ERR;
    if (!total || (cap && !res)) { rr::set_last_error("rr_wpcr_results: null argument"); return RR_ERR; }
    return on_device(w, [&] {
        const std::vector<rr::WpcrResult>& r = w->fetch_results();
        *total = r.size();
        if (const size_t k = std::min(cap, r.size())) std::memcpy(res, r.data(), k * sizeof(rr_wpcr_result));   // (the same layout: blocks_packet.cpp)
    });
}
int rr_debug_wpcr_spectrum(rr_block* b, size_t burst, float* mag, size_t cap, size_t* nbins) {
    auto* w = as<rr::Wpcr>(b, "rr_debug_wpcr_spectrum", NOT_WPCR);
    if (!w) return RR_ERR;
    if (!nbins || (cap && !mag)) { rr::set_last_error("rr_debug_wpcr_spectrum: null argument"); return RR_ERR; }
    return on_device(w, [&] {
        const std::vector<float> m = w->fetch_spectrum(burst);
        *nbins = m.size();
        if (const size_t k = std::min(cap, m.size())) std::memcpy(mag, m.data(), k * sizeof(float));
    });
}
rr_block* rr_stream_to_pdu_create(float threshold, size_t max_size, size_t tail, int flags) {
    if (const char* e = rr::pdu_check(max_size, flags)) return refuse_create(e);
    return make_block([&] { return new rr::StreamToPdu(threshold, max_size, tail, flags); });
}
int rr_stream_to_pdu_push_dev(rr_block* b, const void* d_data, const void* d_trigger, size_t n, void* hip_stream) {
    auto* p = as<rr::StreamToPdu>(b, "rr_stream_to_pdu_push_dev", NOT_PDU);
    if (!p) return RR_ERR;
    if (n && (!d_data || !d_trigger)) { rr::set_last_error("rr_stream_to_pdu_push_dev: null argument"); return RR_ERR; }
    return on_device(p, hip_stream, [&](hipStream_t s) {
        if (dynamic_cast<rr::BurstSaver*>(p)) throw rr::Error("rr_stream_to_pdu_push_dev: a burst saver takes rr_burst_saver_push_dev");
        p->push_dev(d_data, static_cast<const float*>(d_trigger), n, s);
    });
}
// what a call on host data of element size `es` says to a handle of the other kind (a burst saver is fed by its own calls)
static bool pdu_kind_ok(rr::StreamToPdu* p, size_t es, const char* what, const char* msg, bool saver_ok) {
    if (p->es == es && (saver_ok || !dynamic_cast<rr::BurstSaver*>(p))) return true;
    rr::set_last_error(std::string(what) + ": " + msg);
    return false;
}
static const char PDU_NOT_F32[] = "the PDUs are not f32", PDU_NOT_C32[] = "the PDUs are not Complex";
int rr_stream_to_pdu_push(rr_block* b, const float* data, const float* trigger, size_t n) {
    auto* p = as<rr::StreamToPdu>(b, "rr_stream_to_pdu_push", NOT_PDU);
    if (!p || !pdu_kind_ok(p, 4, "rr_stream_to_pdu_push", PDU_NOT_F32, false)) return RR_ERR;
    if (n && (!data || !trigger)) { rr::set_last_error("rr_stream_to_pdu_push: null argument"); return RR_ERR; }
    return guarded([&] { p->push_host(data, trigger, n); });
}
int rr_pdu_records(rr_block* b, rr_pdu_record* rec, size_t cap, size_t* total) {
    auto* p = as<rr::StreamToPdu>(b, "rr_pdu_records", NOT_PDU);
    if (!p) return RR_ERR;
    if (!total || (cap && !rec)) { rr::set_last_error("rr_pdu_records: null argument"); return RR_ERR; }
    return on_device(p, [&] { rr::pdu_copy_out(p->fetch_records(), rec, cap, total); });
}
int rr_pdu_edges(rr_block* b, size_t* pos, unsigned char* val, size_t cap, size_t* total) {
    auto* p = as<rr::StreamToPdu>(b, "rr_pdu_edges", NOT_PDU);
    if (!p) return RR_ERR;
    if (!total || (cap && (!pos || !val))) { rr::set_last_error("rr_pdu_edges: null argument"); return RR_ERR; }
    return on_device(p, [&] { unpack(p->fetch_edges(), 1, pos, val, cap, total); });
}
const void* rr_pdu_arena_dev(rr_block* b, size_t* n_total) {
    auto* p = as<rr::StreamToPdu>(b, "rr_pdu_arena_dev", NOT_PDU);
    if (n_total) *n_total = p ? p->n_total : 0;
    return p ? p->arena_dev() : nullptr;
}
int rr_pdu_fetch(rr_block* b, size_t idx, float* out, size_t cap) {
    auto* p = as<rr::StreamToPdu>(b, "rr_pdu_fetch", NOT_PDU);
    if (!p || !pdu_kind_ok(p, 4, "rr_pdu_fetch", PDU_NOT_F32, true)) return RR_ERR;
    if (cap && !out) { rr::set_last_error("rr_pdu_fetch: null argument"); return RR_ERR; }
    return on_device(p, [&] { p->fetch_pdu(idx, out, cap); });
}
int rr_debug_pdu_ranks(rr_block* b, size_t idx, float* low, float* high) {
    auto* p = as<rr::StreamToPdu>(b, "rr_debug_pdu_ranks", NOT_PDU);
    if (!p) return RR_ERR;
    if (!low || !high) { rr::set_last_error("rr_debug_pdu_ranks: null argument"); return RR_ERR; }
    return on_device(p, [&] { p->fetch_ranks(idx, low, high); });
}
int rr_wpcr_process_pdus(rr_block* wpcr, rr_block* pdus, void* d_syms, void* hip_stream) {
    auto* w = as<rr::Wpcr>(wpcr, "rr_wpcr_process_pdus", NOT_WPCR);
    auto* p = as<rr::StreamToPdu>(pdus, "rr_wpcr_process_pdus", NOT_PDU);
    if (!w || !p) return RR_ERR;
    if (p->es != 4) { rr::set_last_error("wpcr: the PDUs are not f32"); return RR_ERR; }
    return on_device(p, [&] {
        if (w->device != p->device) throw rr::Error("rr_wpcr_process_pdus: the two handles live on different devices");
        std::vector<size_t> starts, lens;
        std::vector<float> mids;
        if (const char* e = rr::pdu_select(p->fetch_records(), p->midpoint, p->n_total, rr::Wpcr::MAX_LEN, starts, lens, mids))
            throw rr::Error(e);
        if (!starts.empty() && !d_syms) throw rr::Error("rr_wpcr_process_pdus: null argument");
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        w->last_stream = s;
        w->process_dev(static_cast<const float*>(p->arena_dev()), p->n_total, starts.data(), lens.data(), p->midpoint ? mids.data() : nullptr, starts.size(),
                       static_cast<float*>(d_syms), s);
    });
}
rr_block* rr_stream_to_pdu_c32_create(float threshold, size_t max_size, size_t tail) {
    if (const char* e = rr::pdu_check(max_size, 0)) return refuse_create(e);
    return make_block([&] { return new rr::StreamToPdu(threshold, max_size, tail, 0, 8); });
}
int rr_stream_to_pdu_push_c32(rr_block* b, const rr_c32* data, const float* trigger, size_t n) {
    auto* p = as<rr::StreamToPdu>(b, "rr_stream_to_pdu_push_c32", NOT_PDU);
    if (!p || !pdu_kind_ok(p, 8, "rr_stream_to_pdu_push_c32", PDU_NOT_C32, false)) return RR_ERR;
    if (n && (!data || !trigger)) { rr::set_last_error("rr_stream_to_pdu_push_c32: null argument"); return RR_ERR; }
    return guarded([&] { p->push_host(data, trigger, n); });
}
int rr_pdu_fetch_c32(rr_block* b, size_t idx, rr_c32* out, size_t cap) {
    auto* p = as<rr::StreamToPdu>(b, "rr_pdu_fetch_c32", NOT_PDU);
    if (!p || !pdu_kind_ok(p, 8, "rr_pdu_fetch_c32", PDU_NOT_C32, true)) return RR_ERR;
    if (cap && !out) { rr::set_last_error("rr_pdu_fetch_c32: null argument"); return RR_ERR; }
    return on_device(p, [&] { p->fetch_pdu(idx, out, cap); });
}
rr_block* rr_delay_create(size_t delay, size_t elem_size) {
    if (const char* e = rr::delay_check(delay, elem_size)) return refuse_create(e);
    return make_block([&] { return new rr::Delay(delay, elem_size); }, RR_TAGS_SHIFT, delay);
}
static const char NOT_SAVER[] = "not a burst saver handle";
rr_block* rr_burst_saver_create(float alpha, float threshold, size_t delay, size_t max_size, size_t tail) {
    if (const char* e = rr::saver_check(alpha, delay, max_size)) return refuse_create(e);
    return make_block([&] { return new rr::BurstSaver(alpha, threshold, delay, max_size, tail); });
}
int rr_burst_saver_push_dev(rr_block* b, const void* d_in, size_t n, void* d_env, void* hip_stream) {
    auto* p = as<rr::BurstSaver>(b, "rr_burst_saver_push_dev", NOT_SAVER);
    if (!p) return RR_ERR;
    if (const char* e = rr::saver_push_check(d_in, n)) { rr::set_last_error(std::string("rr_burst_saver_push_dev: ") + e); return RR_ERR; }
    return on_device(p, hip_stream, [&](hipStream_t s) { p->push_dev(static_cast<const rr::cf*>(d_in), n, static_cast<float*>(d_env), s); });
}
int rr_burst_saver_push(rr_block* b, const rr_c32* in, size_t n, float* env) {
    auto* p = as<rr::BurstSaver>(b, "rr_burst_saver_push", NOT_SAVER);
    if (!p) return RR_ERR;
    if (const char* e = rr::saver_push_check(in, n)) { rr::set_last_error(std::string("rr_burst_saver_push: ") + e); return RR_ERR; }
    return guarded([&] { p->push_host(reinterpret_cast<const rr::cf*>(in), n, env); });
}
int rr_burst_saver_dims(const rr_block* b, size_t n, size_t* tile, size_t* launches) {
    auto* p = as<rr::BurstSaver>(b, "rr_burst_saver_dims", NOT_SAVER);
    if (!p) return RR_ERR;
    if (tile) *tile = rr::IIR_T;
    if (launches) *launches = rr::saver_launches(n, rr::IIR_T);
    return 0;
}
int rr_wpcr_pack_dev(rr_block* wpcr, const void* d_syms, void* d_out, size_t out_cap, size_t* produced, size_t* pdu_start,
                     size_t* pdu_len, size_t cap, size_t* npdus, void* hip_stream) {
    auto* w = as<rr::Wpcr>(wpcr, "rr_wpcr_pack_dev", NOT_WPCR);
    if (!w) return RR_ERR;
    if (!produced || !npdus) { rr::set_last_error("rr_wpcr_pack_dev: null argument"); return RR_ERR; }
    return on_device(w, [&] {
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        w->pack_dev(static_cast<const float*>(d_syms), static_cast<float*>(d_out), out_cap, produced, pdu_start, pdu_len, cap, npdus, s);
        w->last_stream = s;
    });
}
rr_block* rr_nrzi_encode_create(void) {
    return make_block([&] { return new rr::LineCoder("NrziEncode", rr::LINE_NRZI); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_scrambler_g3ruh_create(void) {
    return make_block([&] { return new rr::LineCoder("Scrambler", rr::LINE_SCR); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_hdlc_framer_create(int flags, float lo, float hi) {
    if (const char* e = rr::frame_check_flags(flags)) return refuse_create(e);
    return make_block([&] { return new rr::HdlcFramer(flags, lo, hi); });
}
size_t rr_hdlc_framer_bound(const rr_block* b, const size_t* lens, size_t npackets) {
    auto* f = as<rr::HdlcFramer>(b, "rr_hdlc_framer_bound", NOT_FRAMER);
    if (!f || (npackets && !lens)) return 0;
    return rr::frame_bound(f->flags, lens, npackets);
}
int rr_hdlc_framer_push_dev(rr_block* b, const void* d_bytes, size_t n_bytes, size_t* starts, size_t* lens, size_t npackets,
                            void* d_out, size_t out_cap, void* hip_stream) {
    auto* f = as<rr::HdlcFramer>(b, "rr_hdlc_framer_push_dev", NOT_FRAMER);
    if (!f) return RR_ERR;
    size_t bound = 0;                                  // every refusal before any device is touched
    if (const char* e = rr::frame_check_push(f->flags, n_bytes, starts, lens, npackets, out_cap, &bound)) { rr::set_last_error(e); return RR_ERR; }
    if (npackets && (!d_out || (n_bytes && !d_bytes))) { rr::set_last_error("rr_hdlc_framer_push_dev: null argument"); return RR_ERR; }
    return on_device(f, hip_stream, [&](hipStream_t s) {
        f->push_dev(static_cast<const unsigned char*>(d_bytes), n_bytes, starts, lens, npackets, d_out, out_cap, s);
    });
}
int rr_hdlc_framer_push(rr_block* b, const unsigned char* bytes, size_t n_bytes, size_t* starts, size_t* lens, size_t npackets,
                        void* out, size_t out_cap, size_t* produced) {
    auto* f = as<rr::HdlcFramer>(b, "rr_hdlc_framer_push", NOT_FRAMER);
    if (!f) return RR_ERR;
    if (!produced) { rr::set_last_error("rr_hdlc_framer_push: null argument"); return RR_ERR; }
    size_t bound = 0;
    if (const char* e = rr::frame_check_push(f->flags, n_bytes, starts, lens, npackets, out_cap, &bound)) { rr::set_last_error(e); return RR_ERR; }
    if (npackets && (!out || (n_bytes && !bytes))) { rr::set_last_error("rr_hdlc_framer_push: null argument"); return RR_ERR; }
    return guarded([&] { f->push_host(bytes, n_bytes, starts, lens, npackets, out, out_cap, produced); });
}
int rr_hdlc_framer_records(rr_block* b, rr_frame_record* rec, size_t cap, size_t* total, size_t* produced) {
    auto* f = as<rr::HdlcFramer>(b, "rr_hdlc_framer_records", NOT_FRAMER);
    if (!f) return RR_ERR;
    if (!total || !produced || (cap && !rec)) { rr::set_last_error("rr_hdlc_framer_records: null argument"); return RR_ERR; }
    return on_device(f, [&] {
        rr::frame_copy_out(f->fetch_records(), rec, cap, total);
        *produced = f->produced;
    });
}
int rr_hdlc_framer_dims(const rr_block* b, size_t* tile_bits) {
    auto* f = as<rr::HdlcFramer>(b, "rr_hdlc_framer_dims", NOT_FRAMER);
    if (!f || !tile_bits) { if (f) rr::set_last_error("rr_hdlc_framer_dims: null argument"); return RR_ERR; }
    static_assert(rr::FRAME_T == rr::LINE_T, "one tile length for the stuffing scan and the line coder");
    *tile_bits = rr::FRAME_T;
    return 0;
}
const void* rr_hdlc_framer_produced_dev(rr_block* b) {
    auto* f = as<rr::HdlcFramer>(b, "rr_hdlc_framer_produced_dev", NOT_FRAMER);
    return f ? f->total.p : nullptr;
}
rr_block* rr_hdlc_deframer_create(size_t min_size, size_t max_size, int flags) {
    if (const char* e = rr::hdlc_check_create(min_size, max_size, flags)) return refuse_create(e);
    return make_block([&] { return new rr::HdlcDeframer(min_size, max_size, flags); });
}
int rr_hdlc_deframer_push_dev(rr_block* b, const void* d_bits, size_t n, void* hip_stream) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_deframer_push_dev", NOT_DEFRAMER);
    if (!d) return RR_ERR;
    if (const char* e = rr::hdlc_check_push(d_bits, n)) { rr::set_last_error(e); return RR_ERR; }     // before any device is touched
    return on_device(d, hip_stream, [&](hipStream_t s) { d->push_dev(static_cast<const unsigned char*>(d_bits), n, s); });
}
int rr_hdlc_deframer_push(rr_block* b, const unsigned char* bits, size_t n) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_deframer_push", NOT_DEFRAMER);
    if (!d) return RR_ERR;
    if (const char* e = rr::hdlc_check_push(bits, n)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { d->push_host(bits, n); });
}
int rr_hdlc_frames(rr_block* b, rr_hdlc_frame* rec, size_t cap, size_t* total) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_frames", NOT_DEFRAMER);
    if (!d) return RR_ERR;
    if (!total || (cap && !rec)) { rr::set_last_error("rr_hdlc_frames: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::hdlc_copy_frames(d->fetch_frames(), rec, cap, total); });
}
int rr_hdlc_frame_bytes(rr_block* b, unsigned char* out, size_t cap, size_t* total) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_frame_bytes", NOT_DEFRAMER);
    if (!d) return RR_ERR;
    if (!total || (cap && !out)) { rr::set_last_error("rr_hdlc_frame_bytes: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::hdlc_copy_bytes(d->fetch_bytes(), out, cap, total); });
}
const void* rr_hdlc_bytes_dev(rr_block* b, size_t* n_total) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_bytes_dev", NOT_DEFRAMER);
    if (n_total) *n_total = d ? d->core.arena_len() : 0;
    return d && d->core.arena_len() ? d->core.arena_dev() : nullptr;
}
int rr_hdlc_stats(rr_block* b, unsigned long long* decoded, unsigned long long* crc_error, unsigned long long* bitfixed) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_stats", NOT_DEFRAMER);
    if (!d) return RR_ERR;
    if (!decoded || !crc_error || !bitfixed) { rr::set_last_error("rr_hdlc_stats: null argument"); return RR_ERR; }
    return on_device(d, [&] {
        unsigned long long s[3] = {0, 0, 0};
        d->fetch_stats(s);
        *decoded = s[0]; *crc_error = s[1]; *bitfixed = s[2];
    });
}
int rr_hdlc_deframer_dims(const rr_block* b, size_t* tile_bits, size_t* carry_bits) {
    auto* d = as<rr::HdlcDeframer>(b, "rr_hdlc_deframer_dims", NOT_DEFRAMER);
    if (!d || !tile_bits || !carry_bits) { if (d) rr::set_last_error("rr_hdlc_deframer_dims: null argument"); return RR_ERR; }
    *tile_bits = rr::HDLC_T;
    *carry_bits = rr::hdlc_carry_bits(d->core.max_size);
    return 0;
}
rr_block* rr_kiss_decode_create(size_t max_len) {
    if (const char* e = rr::kiss_check_create(max_len)) return refuse_create(e);
    return make_block([&] { return new rr::KissDecode(max_len); });
}
int rr_kiss_decode_push_dev(rr_block* b, const void* d_bytes, size_t n, void* hip_stream) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_decode_push_dev", NOT_KISSDEC);
    if (!d) return RR_ERR;
    if (const char* e = rr::kiss_check_push(d_bytes, n)) { rr::set_last_error(e); return RR_ERR; }     // before any device is touched
    return on_device(d, hip_stream, [&](hipStream_t s) { d->push_dev(static_cast<const unsigned char*>(d_bytes), n, s); });
}
int rr_kiss_decode_push(rr_block* b, const unsigned char* bytes, size_t n) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_decode_push", NOT_KISSDEC);
    if (!d) return RR_ERR;
    if (const char* e = rr::kiss_check_push(bytes, n)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { d->push_host(bytes, n); });
}
int rr_kiss_packets(rr_block* b, rr_kiss_packet* rec, size_t cap, size_t* total) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_packets", NOT_KISSDEC);
    if (!d) return RR_ERR;
    if (!total || (cap && !rec)) { rr::set_last_error("rr_kiss_packets: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::kiss_copy_out(d->fetch_packets(), rec, cap, total); });
}
int rr_kiss_packet_bytes(rr_block* b, unsigned char* out, size_t cap, size_t* total) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_packet_bytes", NOT_KISSDEC);
    if (!d) return RR_ERR;
    if (!total || (cap && !out)) { rr::set_last_error("rr_kiss_packet_bytes: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::kiss_copy_out(d->fetch_bytes(), out, cap, total); });
}
const void* rr_kiss_packet_bytes_dev(rr_block* b, size_t* n_total) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_packet_bytes_dev", NOT_KISSDEC);
    if (n_total) *n_total = d ? d->arena_len() : 0;
    return d ? d->arena_dev() : nullptr;
}
int rr_kiss_decode_stats(rr_block* b, unsigned long long* five) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_decode_stats", NOT_KISSDEC);
    if (!d) return RR_ERR;
    if (!five) { rr::set_last_error("rr_kiss_decode_stats: null argument"); return RR_ERR; }
    return on_device(d, [&] { d->fetch_stats(five); });
}
int rr_kiss_decode_dims(const rr_block* b, size_t* tile_bytes, size_t* carry_bytes, size_t* launches) {
    auto* d = as<rr::KissDecode>(b, "rr_kiss_decode_dims", NOT_KISSDEC);
    if (!d || !tile_bytes || !carry_bytes || !launches) { if (d) rr::set_last_error("rr_kiss_decode_dims: null argument"); return RR_ERR; }
    *tile_bytes = rr::KISS_T;
    *carry_bytes = d->max_len;
    *launches = rr::KISS_DECODE_LAUNCHES;
    return 0;
}
rr_block* rr_kiss_encode_create(void) {
    return make_block([&] { return new rr::KissEncode(); });
}
size_t rr_kiss_encode_bound(const size_t* lens, size_t npackets) {
    if (npackets && !lens) return 0;
    return rr::kiss_encode_bound(lens, npackets);
}
int rr_kiss_encode_push_dev(rr_block* b, const void* d_bytes, size_t n_bytes, size_t* starts, size_t* lens, const unsigned* ports,
                            size_t npackets, void* d_out, size_t out_cap, void* hip_stream) {
    auto* k = as<rr::KissEncode>(b, "rr_kiss_encode_push_dev", NOT_KISSENC);
    if (!k) return RR_ERR;
    size_t bound = 0;                                  // every refusal before any device is touched
    if (const char* e = rr::kiss_encode_check_push(n_bytes, starts, lens, npackets, out_cap, &bound)) { rr::set_last_error(e); return RR_ERR; }
    if (npackets && (!d_out || (n_bytes && !d_bytes))) { rr::set_last_error("kiss encode: null argument"); return RR_ERR; }
    return on_device(k, hip_stream, [&](hipStream_t s) {
        k->push_dev(static_cast<const unsigned char*>(d_bytes), n_bytes, starts, lens, ports, npackets, d_out, out_cap, s);
    });
}
int rr_kiss_encode_push(rr_block* b, const unsigned char* bytes, size_t n_bytes, size_t* starts, size_t* lens, const unsigned* ports,
                        size_t npackets, unsigned char* out, size_t out_cap, size_t* produced) {
    auto* k = as<rr::KissEncode>(b, "rr_kiss_encode_push", NOT_KISSENC);
    if (!k) return RR_ERR;
    if (!produced) { rr::set_last_error("kiss encode: null argument"); return RR_ERR; }
    size_t bound = 0;
    if (const char* e = rr::kiss_encode_check_push(n_bytes, starts, lens, npackets, out_cap, &bound)) { rr::set_last_error(e); return RR_ERR; }
    if (npackets && (!out || (n_bytes && !bytes))) { rr::set_last_error("kiss encode: null argument"); return RR_ERR; }
    return guarded([&] { k->push_host(bytes, n_bytes, starts, lens, ports, npackets, out, out_cap, produced); });
}
int rr_kiss_encode_records(rr_block* b, rr_kiss_frame_record* rec, size_t cap, size_t* total, size_t* produced) {
    auto* k = as<rr::KissEncode>(b, "rr_kiss_encode_records", NOT_KISSENC);
    if (!k) return RR_ERR;
    if (!total || !produced || (cap && !rec)) { rr::set_last_error("rr_kiss_encode_records: null argument"); return RR_ERR; }
    return on_device(k, [&] {
        rr::kiss_copy_out(k->fetch_records(), rec, cap, total);
        *produced = k->produced;
    });
}
int rr_kiss_encode_dims(const rr_block* b, size_t* tile_bytes, size_t* launches) {
    auto* k = as<rr::KissEncode>(b, "rr_kiss_encode_dims", NOT_KISSENC);
    if (!k || !tile_bytes || !launches) { if (k) rr::set_last_error("rr_kiss_encode_dims: null argument"); return RR_ERR; }
    *tile_bytes = rr::KISS_T;
    *launches = rr::KISS_ENCODE_LAUNCHES;
    return 0;
}
int rr_kiss_encode_frames(rr_block* kiss, rr_block* src, const unsigned* port_of_stream, size_t nports, void* d_out, size_t out_cap,
                          void* hip_stream) {
    auto* k = as<rr::KissEncode>(kiss, "rr_kiss_encode_frames", NOT_KISSENC);
    if (!k) return RR_ERR;
    auto* d = src ? dynamic_cast<rr::HdlcDeframer*>(src->b.get()) : nullptr;
    auto* r = src ? dynamic_cast<rr::HdlcReceiver*>(src->b.get()) : nullptr;
    if (!d && !r) { rr::set_last_error("rr_kiss_encode_frames: not an hdlc deframer or receiver handle"); return RR_ERR; }
    return on_device(k, [&] {
        if (k->device != (d ? d->device : r->device)) throw rr::Error("rr_kiss_encode_frames: the two handles live on different devices");
        std::vector<size_t> starts, lens;
        std::vector<unsigned> ports;
        if (d) {
            for (const rr_hdlc_frame& f : d->fetch_frames()) { starts.push_back((size_t)f.start); lens.push_back(f.len); }
        } else {
            if (r->core.nstreams > nports || !port_of_stream) throw rr::Error("kiss encode: port_of_stream shorter than the receiver's streams");
            for (const rr_hdlc_stream_frame& f : r->fetch_frames()) {
                starts.push_back((size_t)f.start); lens.push_back(f.len); ports.push_back(port_of_stream[f.stream]);
            }
        }
        rr::HdlcCore& core = d ? d->core : r->core;
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        k->last_stream = s;
        k->push_dev(core.arena_dev(), core.arena_len(), starts.data(), lens.data(), d ? nullptr : ports.data(), starts.size(), d_out, out_cap, s);
    });
}
int rr_hdlc_framer_push_kiss(rr_block* framer, rr_block* kiss_decode, void* d_out, size_t out_cap, void* hip_stream) {
    auto* f = as<rr::HdlcFramer>(framer, "rr_hdlc_framer_push_kiss", NOT_FRAMER);
    auto* k = as<rr::KissDecode>(kiss_decode, "rr_hdlc_framer_push_kiss", NOT_KISSDEC);
    if (!f || !k) return RR_ERR;
    return on_device(f, [&] {
        if (f->device != k->device) throw rr::Error("rr_hdlc_framer_push_kiss: the two handles live on different devices");
        std::vector<size_t> starts, lens;
        for (const rr_kiss_packet& p : k->fetch_packets()) { starts.push_back((size_t)p.start); lens.push_back(p.len); }
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        f->last_stream = s;
        f->push_dev(k->arena_dev(), k->arena_len(), starts.data(), lens.data(), starts.size(), d_out, out_cap, s);
    });
}
rr_block* rr_pwm_decoder_create(float high_threshold, float low_threshold, size_t short_width, size_t long_width, size_t pulse_tolerance,
                                size_t frame_gap, size_t reset_gap, size_t frame_bits, size_t max_frame_bits, size_t max_distinct_frames,
                                size_t min_repeats, int flags, size_t in_elem_size) {
    if (const char* e = rr::pwm_check_create(high_threshold, low_threshold, short_width, long_width, pulse_tolerance, frame_gap, reset_gap,
                                             frame_bits, max_frame_bits, max_distinct_frames, min_repeats, flags, in_elem_size))
        return refuse_create(e);
    const rr::PwmCfg c = rr::pwm_cfg(high_threshold, low_threshold, short_width, long_width, pulse_tolerance, frame_gap, reset_gap, frame_bits,
                                     max_frame_bits, max_distinct_frames, min_repeats, flags);
    return make_block([&] { return new rr::PwmDecoder(c, in_elem_size); });
}
int rr_pwm_decoder_push_dev(rr_block* b, const void* d_samples, size_t n, void* hip_stream) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_decoder_push_dev", NOT_PWM);
    if (!d) return RR_ERR;
    if (const char* e = rr::pwm_check_push(d_samples, n, d->flushed)) { rr::set_last_error(e); return RR_ERR; }     // before any device is touched
    return on_device(d, hip_stream, [&](hipStream_t s) { d->push_dev(d_samples, n, s); });
}
int rr_pwm_decoder_push(rr_block* b, const void* samples, size_t n) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_decoder_push", NOT_PWM);
    if (!d) return RR_ERR;
    if (const char* e = rr::pwm_check_push(samples, n, d->flushed)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { d->push_host(samples, n); });
}
int rr_pwm_decoder_flush(rr_block* b, void* hip_stream) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_decoder_flush", NOT_PWM);
    if (!d) return RR_ERR;
    if (const char* e = rr::pwm_check_push(nullptr, 0, d->flushed)) { rr::set_last_error(e); return RR_ERR; }
    return on_device(d, hip_stream, [&](hipStream_t s) { d->flush(s); });
}
int rr_pwm_frames(rr_block* b, rr_pwm_frame* rec, size_t cap, size_t* total) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_frames", NOT_PWM);
    if (!d) return RR_ERR;
    if (!total || (cap && !rec)) { rr::set_last_error("rr_pwm_frames: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::pwm_copy_frames(d->fetch_frames(), rec, cap, total); });
}
int rr_pwm_frame_bits(rr_block* b, unsigned char* out, size_t cap, size_t* total) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_frame_bits", NOT_PWM);
    if (!d) return RR_ERR;
    if (!total || (cap && !out)) { rr::set_last_error("rr_pwm_frame_bits: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::pwm_copy_bits(d->fetch_bits(), out, cap, total); });
}
const void* rr_pwm_bits_dev(rr_block* b, size_t* n_total) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_bits_dev", NOT_PWM);
    if (n_total) *n_total = 0;
    if (!d) return nullptr;
    size_t k = 0;
    if (on_device(d, [&] { k = d->fetch_bits().size(); }) != 0) return nullptr;
    if (n_total) *n_total = k;
    return k ? d->arena.p : nullptr;
}
int rr_pwm_decoder_dims(const rr_block* b, size_t* tile_samples) {
    auto* d = as<rr::PwmDecoder>(b, "rr_pwm_decoder_dims", NOT_PWM);
    if (!d || !tile_samples) { if (d) rr::set_last_error("rr_pwm_decoder_dims: null argument"); return RR_ERR; }
    *tile_samples = rr::PWM_T;
    return 0;
}
rr_block* rr_hdlc_receiver_create(size_t nstreams, int bit_flags, unsigned long long mask, unsigned long long seed, unsigned len,
                                  size_t min_size, size_t max_size, int hdlc_flags) {
    if (const char* e = rr::hdlcrx_check_create(nstreams, bit_flags, seed, len, min_size, max_size, hdlc_flags)) return refuse_create(e);
    return make_block([&] { return new rr::HdlcReceiver(nstreams, bit_flags, mask, seed, len, min_size, max_size, hdlc_flags); });
}
int rr_hdlc_receiver_push_dev(rr_block* b, const void* d_syms, size_t stride, size_t n_cap, const void* d_counts, void* hip_stream) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_push_dev", NOT_RECEIVER);
    if (!d) return RR_ERR;
    if (const char* e = rr::hdlcrx_check_push(d->core.nstreams, d_syms, stride, n_cap)) { rr::set_last_error(e); return RR_ERR; }   // before any device is touched
    return on_device(d, hip_stream, [&](hipStream_t s) {
        d->push_dev(static_cast<const float*>(d_syms), stride, n_cap, static_cast<const unsigned long long*>(d_counts), s);
    });
}
int rr_hdlc_receiver_push(rr_block* b, const float* syms, size_t stride, size_t n_cap, const size_t* counts) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_push", NOT_RECEIVER);
    if (!d) return RR_ERR;
    if (const char* e = rr::hdlcrx_check_push(d->core.nstreams, syms, stride, n_cap)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { d->push_host(syms, stride, n_cap, counts); });
}
int rr_hdlc_receiver_frames(rr_block* b, rr_hdlc_stream_frame* rec, size_t cap, size_t* total) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_frames", NOT_RECEIVER);
    if (!d) return RR_ERR;
    if (!total || (cap && !rec)) { rr::set_last_error("rr_hdlc_receiver_frames: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::hdlcrx_copy_frames(d->fetch_frames(), rec, cap, total); });
}
int rr_hdlc_receiver_frame_bytes(rr_block* b, unsigned char* out, size_t cap, size_t* total) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_frame_bytes", NOT_RECEIVER);
    if (!d) return RR_ERR;
    if (!total || (cap && !out)) { rr::set_last_error("rr_hdlc_receiver_frame_bytes: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::hdlc_copy_bytes(d->fetch_bytes(), out, cap, total); });
}
const void* rr_hdlc_receiver_bytes_dev(rr_block* b, size_t* n_total) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_bytes_dev", NOT_RECEIVER);
    if (n_total) *n_total = d ? d->core.arena_len() : 0;
    return d ? d->core.arena_dev() : nullptr;
}
int rr_hdlc_receiver_stats(rr_block* b, unsigned long long* decoded, unsigned long long* crc_error, unsigned long long* bitfixed, size_t cap,
                           size_t* total) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_stats", NOT_RECEIVER);
    if (!d) return RR_ERR;
    if (!total) { rr::set_last_error("rr_hdlc_receiver_stats: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] {
        const std::vector<unsigned long long> s = d->fetch_stats();
        rr::hdlcrx_copy_u64(s, 0, 3, decoded, cap, total);
        rr::hdlcrx_copy_u64(s, 1, 3, crc_error, cap, total);
        rr::hdlcrx_copy_u64(s, 2, 3, bitfixed, cap, total);
    });
}
int rr_hdlc_receiver_consumed(rr_block* b, unsigned long long* symbols, size_t cap, size_t* total) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_consumed", NOT_RECEIVER);
    if (!d) return RR_ERR;
    if (!total || (cap && !symbols)) { rr::set_last_error("rr_hdlc_receiver_consumed: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::hdlcrx_copy_u64(d->fetch_consumed(), 0, 1, symbols, cap, total); });
}
int rr_hdlc_receiver_dims(const rr_block* b, size_t* tile_bits, size_t* carry_bits) {
    auto* d = as<rr::HdlcReceiver>(b, "rr_hdlc_receiver_dims", NOT_RECEIVER);
    if (!d || !tile_bits || !carry_bits) { if (d) rr::set_last_error("rr_hdlc_receiver_dims: null argument"); return RR_ERR; }
    *tile_bits = rr::HDLC_T;
    *carry_bits = rr::hdlc_carry_bits(d->core.max_size);
    return 0;
}
// Il2pReceiver: BinarySlicer -> [XorConst(1)] -> CorrelateAccessCodeTag(SYNC_WORD) -> Il2pDeframer x nstreams (binary_slicer.rs:17-19,
// correlate_access_code.rs:93-118, il2p_deframer.rs:172-237, 247-319; examples/il2p-1200-rx.rs:118-137)
rr_block* rr_il2p_receiver_create(size_t nstreams, int bit_flags, size_t allowed_diffs) {
    if (const char* e = rr::il2p_check_create(nstreams, bit_flags)) return refuse_create(e);
    return make_block([&] { return new rr::Il2pReceiver(nstreams, bit_flags, allowed_diffs); });
}
// one Il2pDeframer::work() sweep of every stream (il2p_deframer.rs:172-237) over symbols that are already on the device
int rr_il2p_receiver_push_dev(rr_block* b, const void* d_syms, size_t stride, size_t n_cap, const void* d_counts, void* hip_stream) {
    auto* d = as<rr::Il2pReceiver>(b, "rr_il2p_receiver_push_dev", NOT_IL2P);
    if (!d) return RR_ERR;
    if (const char* e = rr::il2p_check_push(d->nstreams, d_syms, stride, n_cap)) { rr::set_last_error(e); return RR_ERR; }   // before any device is touched
    return on_device(d, hip_stream, [&](hipStream_t s) {
        d->push_dev(static_cast<const float*>(d_syms), stride, n_cap, static_cast<const unsigned long long*>(d_counts), s);
    });
}
int rr_il2p_receiver_push(rr_block* b, const float* syms, size_t stride, size_t n_cap, const size_t* counts) {
    auto* d = as<rr::Il2pReceiver>(b, "rr_il2p_receiver_push", NOT_IL2P);
    if (!d) return RR_ERR;
    if (const char* e = rr::il2p_check_push(d->nstreams, syms, stride, n_cap)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { d->push_host(syms, stride, n_cap, counts); });
}
// what il2p_deframer.rs:206-213 parses (and :221-231 only logs): the headers that completed inside the most recent push
int rr_il2p_receiver_headers(rr_block* b, rr_il2p_header* rec, size_t cap, size_t* total) {
    auto* d = as<rr::Il2pReceiver>(b, "rr_il2p_receiver_headers", NOT_IL2P);
    if (!d) return RR_ERR;
    if (!total || (cap && !rec)) { rr::set_last_error("rr_il2p_receiver_headers: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::il2p_copy_headers(d->fetch_headers(), rec, cap, total); });
}
// il2p_deframer.rs:160 (decoded) and the tags of correlate_access_code.rs:110-116, per stream
int rr_il2p_receiver_stats(rr_block* b, unsigned long long* headers, unsigned long long* syncs, size_t cap, size_t* total) {
    auto* d = as<rr::Il2pReceiver>(b, "rr_il2p_receiver_stats", NOT_IL2P);
    if (!d) return RR_ERR;
    if (!total) { rr::set_last_error("rr_il2p_receiver_stats: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] {
        const std::vector<unsigned long long> s = d->fetch_stats();
        rr::il2p_copy_u64(s, 0, 2, headers, cap, total);
        rr::il2p_copy_u64(s, 1, 2, syncs, cap, total);
    });
}
int rr_il2p_receiver_consumed(rr_block* b, unsigned long long* symbols, size_t cap, size_t* total) {
    auto* d = as<rr::Il2pReceiver>(b, "rr_il2p_receiver_consumed", NOT_IL2P);
    if (!d) return RR_ERR;
    if (!total || (cap && !symbols)) { rr::set_last_error("rr_il2p_receiver_consumed: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(d, [&] { rr::il2p_copy_u64(d->fetch_consumed(), 0, 1, symbols, cap, total); });
}
int rr_il2p_receiver_dims(const rr_block* b, size_t* tile_bits, size_t* carry_bits) {
    auto* d = as<rr::Il2pReceiver>(b, "rr_il2p_receiver_dims", NOT_IL2P);
    if (!d || !tile_bits || !carry_bits) { if (d) rr::set_last_error("rr_il2p_receiver_dims: null argument"); return RR_ERR; }
    *tile_bits = rr::IL2P_T;
    *carry_bits = rr::IL2P_CARRY;
    return 0;
}
rr_block* rr_symbol_sync_create(float sps, float max_deviation, const float* taps, size_t ntaps, size_t nstreams) {
    if (const char* e = rr::symsync_check(sps, max_deviation, taps, ntaps, nstreams)) return refuse_create(e);
    return make_block([&] { return new rr::SymbolSync(sps, max_deviation, taps, ntaps, nstreams); });
}
int rr_symbol_sync_push_dev(rr_block* b, const void* d_in, size_t in_stride, size_t n, void* d_syms, void* d_clock, size_t out_stride,
                            void* hip_stream) {
    auto* y = as<rr::SymbolSync>(b, "rr_symbol_sync_push_dev", NOT_SYNC);
    if (!y) return RR_ERR;
    if (const char* e = rr::symsync_check_push(d_in, in_stride, n, d_syms, out_stride)) { rr::set_last_error(e); return RR_ERR; }
    return on_device(y, hip_stream, [&](hipStream_t s) {
        y->push_dev(static_cast<const float*>(d_in), in_stride, n, static_cast<float*>(d_syms), static_cast<float*>(d_clock), out_stride, s);
    });
}
int rr_symbol_sync_push(rr_block* b, const float* in, size_t in_stride, size_t n, float* syms, float* clock, size_t out_stride,
                        size_t* produced) {
    auto* y = as<rr::SymbolSync>(b, "rr_symbol_sync_push", NOT_SYNC);
    if (!y) return RR_ERR;
    if (!produced) { rr::set_last_error("rr_symbol_sync_push: null argument"); return RR_ERR; }
    if (const char* e = rr::symsync_check_push(in, in_stride, n, syms, out_stride)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { y->push_host(in, in_stride, n, syms, clock, out_stride, produced); });
}
int rr_symbol_sync_produced(rr_block* b, size_t* produced, size_t cap, size_t* total) {
    auto* y = as<rr::SymbolSync>(b, "rr_symbol_sync_produced", NOT_SYNC);
    if (!y) return RR_ERR;
    if (!total || (cap && !produced)) { rr::set_last_error("rr_symbol_sync_produced: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(y, [&] { rr::symsync_copy_counts(y->fetch_counts(), produced, cap, total); });
}
const void* rr_symbol_sync_counts_dev(rr_block* b) {
    auto* y = as<rr::SymbolSync>(b, "rr_symbol_sync_counts_dev", NOT_SYNC);
    return y ? y->count.p : nullptr;
}
int rr_symbol_sync_dims(const rr_block* b, size_t* streams_per_wave) {
    auto* y = as<rr::SymbolSync>(b, "rr_symbol_sync_dims", NOT_SYNC);
    if (!y || !streams_per_wave) { if (y) rr::set_last_error("rr_symbol_sync_dims: null argument"); return RR_ERR; }
    *streams_per_wave = (size_t)y->spw;
    return 0;
}
int rr_debug_symbol_sync_state(rr_block* b, size_t stream, float* four, int* last_sign, float* hist, size_t cap, size_t* nhist) {
    auto* y = as<rr::SymbolSync>(b, "rr_debug_symbol_sync_state", NOT_SYNC);
    if (!y) return RR_ERR;
    if (!four || !last_sign || !nhist || (cap && !hist)) { rr::set_last_error("rr_debug_symbol_sync_state: null argument"); return RR_ERR; }
    return on_device(y, [&] {
        const rr::SyncState s = y->fetch_state(stream);
        four[0] = s.clock; four[1] = s.stream_pos; four[2] = s.last_sym_boundary_pos; four[3] = s.next_sym_middle;
        *last_sign = s.last_sign;
        const size_t nh = (size_t)y->prm.ntaps - 1;
        *nhist = nh;
        for (size_t i = 0; i < nh && i < cap; i++) hist[i] = s.hist[nh - 1 - i];       // (the device keeps it newest first)
    });
}
rr_block* rr_afsk_demod_create(size_t nstreams, size_t hilbert_ntaps, int window, float window_parm, float gain, const float* taps,
                               size_t ntaps, float offset) {
    if (const char* e = rr::afsk_check(nstreams, hilbert_ntaps, window, window_parm, gain, taps, ntaps, offset)) return refuse_create(e);
    return make_block([&] { return new rr::AfskDemod(nstreams, hilbert_ntaps, window, window_parm, gain, taps, ntaps, offset); });
}
int rr_afsk_demod_push_dev(rr_block* b, const void* d_in, size_t in_stride, size_t n, void* d_out, size_t out_stride, size_t* produced,
                           void* hip_stream) {
    auto* y = as<rr::AfskDemod>(b, "rr_afsk_demod_push_dev", NOT_AFSK);
    if (!y) return RR_ERR;
    if (produced) *produced = 0;
    if (const char* e = rr::afsk_check_push(y->nstreams, d_in, in_stride, n, d_out, out_stride)) { rr::set_last_error(e); return RR_ERR; }
    return on_device(y, hip_stream, [&](hipStream_t s) {
        const size_t k = y->push_dev(static_cast<const float*>(d_in), in_stride, n, static_cast<float*>(d_out), out_stride, s);
        if (produced) *produced = k;
    });
}
int rr_afsk_demod_push(rr_block* b, const float* in, size_t in_stride, size_t n, float* out, size_t out_stride, size_t* produced) {
    auto* y = as<rr::AfskDemod>(b, "rr_afsk_demod_push", NOT_AFSK);
    if (!y) return RR_ERR;
    if (produced) *produced = 0;
    if (const char* e = rr::afsk_check_push(y->nstreams, in, in_stride, n, out, out_stride)) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] {
        const size_t k = y->push_host(in, in_stride, n, out, out_stride);
        if (produced) *produced = k;
    });
}
int rr_afsk_demod_dims(const rr_block* b, size_t* tile_samples, size_t* carry_samples) {
    auto* y = as<rr::AfskDemod>(b, "rr_afsk_demod_dims", NOT_AFSK);
    if (!y || !tile_samples || !carry_samples) { if (y) rr::set_last_error("rr_afsk_demod_dims: null argument"); return RR_ERR; }
    *tile_samples = (size_t)rr::AFSK_TILE;
    *carry_samples = (size_t)y->g.C;
    return 0;
}
rr_block* rr_am_demod_create(size_t nstreams, const float* taps, size_t ntaps, size_t interp, size_t deci, float scale) {
    if (const char* e = rr::am_check(nstreams, taps, ntaps, interp, deci, scale)) return refuse_create(e);
    return make_block([&] { return new rr::AmDemod(nstreams, taps, ntaps, interp, deci, scale); });
}
int rr_am_demod_push_dev(rr_block* b, const void* d_in, size_t in_stride, size_t n, void* d_out, size_t out_stride, size_t* produced,
                         void* hip_stream) {
    auto* y = as<rr::AmDemod>(b, "rr_am_demod_push_dev", NOT_AM);
    if (!y) return RR_ERR;
    size_t k = 0;
    const char* e = rr::am_check_push(y->nstreams, y->g, y->e, d_in, in_stride, n, d_out, out_stride, &k);
    if (produced) *produced = k;
    if (e) { rr::set_last_error(e); return RR_ERR; }
    return on_device(y, hip_stream, [&](hipStream_t s) {
        y->push_dev(static_cast<const rr::cf*>(d_in), in_stride, n, static_cast<float*>(d_out), out_stride, s);
    });
}
int rr_am_demod_push(rr_block* b, const rr_c32* in, size_t in_stride, size_t n, float* out, size_t out_stride, size_t* produced) {
    auto* y = as<rr::AmDemod>(b, "rr_am_demod_push", NOT_AM);
    if (!y) return RR_ERR;
    size_t k = 0;
    const char* e = rr::am_check_push(y->nstreams, y->g, y->e, in, in_stride, n, out, out_stride, &k);
    if (produced) *produced = k;
    if (e) { rr::set_last_error(e); return RR_ERR; }
    return guarded([&] { y->push_host(reinterpret_cast<const rr::cf*>(in), in_stride, n, out, out_stride); });
}
int rr_am_demod_dims(const rr_block* b, size_t* tile_outputs, size_t* carry_samples) {
    auto* y = as<rr::AmDemod>(b, "rr_am_demod_dims", NOT_AM);
    if (!y || !tile_outputs || !carry_samples) { if (y) rr::set_last_error("rr_am_demod_dims: null argument"); return RR_ERR; }
    *tile_outputs = (size_t)y->g.T;
    *carry_samples = (size_t)y->g.C;
    return 0;
}
rr_block* rr_fsk_tx_create(int mode, size_t interp1, size_t deci1, float lo, float hi, unsigned long long k1_bits, float gain,
                           size_t interp2, size_t deci2, unsigned long long k2_bits) {
    const double k1 = f64_from_bits(k1_bits), k2 = f64_from_bits(k2_bits);
    if (const char* e = rr::fsk_check(mode, interp1, deci1, lo, hi, k1, gain, interp2, deci2, k2)) return refuse_create(e);
    return make_block([&] { return new rr::FskTx(mode, interp1, deci1, lo, hi, k1, gain, interp2, deci2, k2); });
}
int rr_fsk_tx_count(const rr_block* b, size_t n_bits, size_t* n_audio, size_t* n_out) {
    auto* y = as<rr::FskTx>(b, "rr_fsk_tx_count", NOT_FSK);
    if (!y) return RR_ERR;
    return guarded([&] {
        const rr::FskPush u = y->count(n_bits);
        if (n_audio) *n_audio = (size_t)u.na;
        if (n_out) *n_out = (size_t)u.no;
    });
}
int rr_fsk_tx_push_dev(rr_block* b, const void* d_bits, size_t n_bits, void* d_out, size_t out_cap, void* d_audio, size_t audio_cap,
                       size_t* n_out, size_t* n_audio, void* hip_stream) {
    auto* y = as<rr::FskTx>(b, "rr_fsk_tx_push_dev", NOT_FSK);
    if (!y) return RR_ERR;
    if (n_out) *n_out = 0;
    if (n_audio) *n_audio = 0;
    if (const char* e = rr::fsk_check_push(y->mode, y->pos, y->r1, y->r2, d_bits, n_bits, d_out, out_cap, d_audio, audio_cap, nullptr)) {
        rr::set_last_error(e);
        return RR_ERR;
    }
    return on_device(y, hip_stream, [&](hipStream_t s) {
        const rr::FskPush u = y->push_dev(static_cast<const unsigned char*>(d_bits), n_bits, static_cast<rr::cf*>(d_out), out_cap,
                                          static_cast<float*>(d_audio), audio_cap, s);
        if (n_out) *n_out = (size_t)u.no;
        if (n_audio) *n_audio = (size_t)u.na;
    });
}
int rr_fsk_tx_push(rr_block* b, const void* bits, size_t n_bits, rr_c32* out, size_t out_cap, float* audio, size_t audio_cap,
                   size_t* n_out, size_t* n_audio) {
    auto* y = as<rr::FskTx>(b, "rr_fsk_tx_push", NOT_FSK);
    if (!y) return RR_ERR;
    if (n_out) *n_out = 0;
    if (n_audio) *n_audio = 0;
    if (const char* e = rr::fsk_check_push(y->mode, y->pos, y->r1, y->r2, bits, n_bits, out, out_cap, audio, audio_cap, nullptr)) {
        rr::set_last_error(e);
        return RR_ERR;
    }
    return guarded([&] {
        const rr::FskPush u = y->push_host(static_cast<const unsigned char*>(bits), n_bits, reinterpret_cast<rr::cf*>(out), out_cap, audio, audio_cap);
        if (n_out) *n_out = (size_t)u.no;
        if (n_audio) *n_audio = (size_t)u.na;
    });
}
int rr_fsk_tx_dims(const rr_block* b, size_t* audio_tile, size_t* out_tile, size_t* scan_chunk_tiles) {
    auto* y = as<rr::FskTx>(b, "rr_fsk_tx_dims", NOT_FSK);
    if (!y || !audio_tile || !out_tile || !scan_chunk_tiles) { if (y) rr::set_last_error("rr_fsk_tx_dims: null argument"); return RR_ERR; }
    *audio_tile = (size_t)rr::FSK_T;
    *out_tile = (size_t)rr::FSK_OT;
    *scan_chunk_tiles = (size_t)rr::FSK_SCAN_CHUNK;
    return 0;
}
rr_block* rr_fsk_tx_multi_create(size_t nstreams, int mode, size_t interp1, size_t deci1, float lo, float hi, unsigned long long k1_bits,
                                 float gain, size_t interp2, size_t deci2, unsigned long long k2_bits) {
    const double k1 = f64_from_bits(k1_bits), k2 = f64_from_bits(k2_bits);
    if (const char* e = rr::fsk_multi_check(nstreams, mode, interp1, deci1, lo, hi, k1, gain, interp2, deci2, k2)) return refuse_create(e);
    return make_block([&] { return new rr::FskTxMulti(nstreams, mode, interp1, deci1, lo, hi, k1, gain, interp2, deci2, k2); });
}
int rr_fsk_tx_multi_bound(const rr_block* b, size_t n_cap, size_t* audio_cap, size_t* out_cap) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_bound", NOT_FSKM);
    if (!y) return RR_ERR;
    size_t ac = 0, oc = 0;
    rr::fsk_multi_bound(y->r1, y->r2, n_cap, &ac, &oc);
    if (audio_cap) *audio_cap = ac;
    if (out_cap) *out_cap = oc;
    return 0;
}
int rr_fsk_tx_multi_push_dev(rr_block* b, const void* d_bits, size_t bits_stride, size_t n_cap, const void* d_counts, void* d_out,
                             size_t out_stride, void* d_audio, size_t audio_stride, void* hip_stream) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_push_dev", NOT_FSKM);
    if (!y) return RR_ERR;
    if (const char* e = rr::fsk_multi_check_push(y->mode, y->nstreams, y->r1, y->r2, y->bits_bound, d_bits, bits_stride, n_cap, d_out,
                                                 out_stride, d_audio, audio_stride, nullptr, nullptr)) {   // before any device is touched
        rr::set_last_error(e);
        return RR_ERR;
    }
    return on_device(y, hip_stream, [&](hipStream_t s) {
        y->push_dev(static_cast<const unsigned char*>(d_bits), bits_stride, n_cap, static_cast<const unsigned long long*>(d_counts),
                    static_cast<rr::cf*>(d_out), out_stride, static_cast<float*>(d_audio), audio_stride, s);
    });
}
int rr_fsk_tx_multi_push(rr_block* b, const unsigned char* bits, size_t bits_stride, size_t n_cap, const size_t* counts, rr_c32* out,
                         size_t out_stride, float* audio, size_t audio_stride, size_t* n_out, size_t* n_audio) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_push", NOT_FSKM);
    if (!y) return RR_ERR;
    for (size_t c = 0; c < y->nstreams; c++) {
        if (n_out) n_out[c] = 0;
        if (n_audio) n_audio[c] = 0;
    }
    if (const char* e = rr::fsk_multi_check_push(y->mode, y->nstreams, y->r1, y->r2, y->bits_bound, bits, bits_stride, n_cap, out, out_stride,
                                                 audio, audio_stride, nullptr, nullptr)) {
        rr::set_last_error(e);
        return RR_ERR;
    }
    return guarded([&] { y->push_host(bits, bits_stride, n_cap, counts, reinterpret_cast<rr::cf*>(out), out_stride, audio, audio_stride, n_out, n_audio); });
}
int rr_fsk_tx_multi_counts(rr_block* b, size_t* n_audio, size_t* n_out, size_t cap, size_t* total) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_counts", NOT_FSKM);
    if (!y) return RR_ERR;
    if (!total) { rr::set_last_error("rr_fsk_tx_multi_counts: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(y, [&] {
        const std::vector<unsigned long long>& k = y->fetch_counts();
        *total = y->nstreams;
        for (size_t c = 0; c < y->nstreams && c < cap; c++) {
            if (n_audio) n_audio[c] = (size_t)k[c];
            if (n_out) n_out[c] = (size_t)k[y->nstreams + c];
        }
    });
}
const void* rr_fsk_tx_multi_counts_dev(rr_block* b) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_counts_dev", NOT_FSKM);
    return y ? y->made.p : nullptr;
}
int rr_fsk_tx_multi_positions(rr_block* b, unsigned long long* bits, unsigned long long* audio, unsigned long long* out, size_t cap,
                              size_t* total) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_positions", NOT_FSKM);
    if (!y) return RR_ERR;
    if (!total) { rr::set_last_error("rr_fsk_tx_multi_positions: null argument"); return RR_ERR; }
    *total = 0;
    return on_device(y, [&] {
        const std::vector<rr::FskStream> st = y->fetch_state();
        *total = st.size();
        for (size_t c = 0; c < st.size() && c < cap; c++) {
            if (bits) bits[c] = st[c].pos.bits;
            if (audio) audio[c] = st[c].pos.audio;
            if (out) out[c] = st[c].pos.out;
        }
    });
}
int rr_fsk_tx_multi_dims(const rr_block* b, size_t* audio_tile, size_t* out_tile, size_t* scan_chunk_tiles) {
    auto* y = as<rr::FskTxMulti>(b, "rr_fsk_tx_multi_dims", NOT_FSKM);
    if (!y || !audio_tile || !out_tile || !scan_chunk_tiles) { if (y) rr::set_last_error("rr_fsk_tx_multi_dims: null argument"); return RR_ERR; }
    *audio_tile = (size_t)rr::FSK_T;
    *out_tile = (size_t)rr::FSK_OT;
    *scan_chunk_tiles = (size_t)rr::FSK_SCAN_CHUNK;
    return 0;
}
rr_block* rr_airspy_decode_create(void) {
    return make_block([&] { return new rr::AirspyDecode(); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_rtlsdr_decode_create(void) {
    return make_block([&] { return new rr::RtlSdrDecode(); });
}
rr_block* rr_quaddemod_create(float gain, int atan2_mode) {
    return make_block([&] { return new rr::QuadDemod(gain, atan2_mode); });
}
rr_block* rr_hilbert_create(size_t ntaps, int window, float window_parm) {
    return make_block([&] { return new rr::Hilbert(ntaps, window, window_parm); }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_fm_chain_create(const rr_c32* taps, size_t ntaps, size_t interp, size_t deci, float gain, int atan2_mode) {
    return make_block([&] { return rr::make_fm_chain(taps, ntaps, interp, deci, gain, atan2_mode, false, nullptr, 0); });
}
rr_block* rr_fir_fftfilter_create(const rr_c32* fir_taps, size_t fir_ntaps, const rr_c32* fft_taps, size_t fft_ntaps) {
    return make_block([&] {
        const std::vector<rr_c32> g = rr::FftFilter::composite(fir_taps, fir_ntaps, fft_taps, fft_ntaps);
        std::unique_ptr<rr::FftFilter> f(new rr::FftFilter(g.data(), g.size(), false, 14, false, fir_ntaps - 1));
        f->set_stage_taps(fir_taps, fir_ntaps, fft_taps, fft_ntaps);
        f->ref_blocks_on(g.data());
        return f.release();
    }, RR_TAGS_FORWARD, 1);
}
rr_block* rr_fir_fm_chain_create(const rr_c32* fir_taps, size_t fir_ntaps, const rr_c32* fft_taps, size_t fft_ntaps,
                                 size_t interp, size_t deci, float gain, int atan2_mode) {
    return make_block([&] {
        if (!fir_taps || fir_ntaps == 0) throw rr::Error("FirFilter: empty taps");
        return rr::make_fm_chain(fft_taps, fft_ntaps, interp, deci, gain, atan2_mode, false, fir_taps, fir_ntaps);
    });
}
rr_block* rr_audio_chain_create(const float* taps, size_t ntaps, size_t interp, size_t deci, float scale) {
    return make_block([&] { return rr::make_audio_chain(taps, ntaps, interp, deci, scale); });
}
rr_block* rr_fm_multi_create(const rr_c32* taps, size_t nchan, size_t ntaps, size_t interp, size_t deci, float gain,
                             int atan2_mode) {
    return make_block([&] { return rr::make_fm_multi(taps, nchan, ntaps, interp, deci, gain, atan2_mode, false); });
}
rr_block* rr_fm_multi_u8_create(const rr_c32* taps, size_t nchan, size_t ntaps, size_t interp, size_t deci, float gain,
                                int atan2_mode) {
    return make_block([&] { return rr::make_fm_multi(taps, nchan, ntaps, interp, deci, gain, atan2_mode, true); });
}
rr_block* rr_channelizer_create(const rr_c32* taps, size_t nchan, size_t ntaps, size_t interp, size_t deci) {
    return make_block([&] { return rr::make_channelizer(taps, nchan, ntaps, interp, deci, false); });
}
rr_block* rr_channelizer_u8_create(const rr_c32* taps, size_t nchan, size_t ntaps, size_t interp, size_t deci) {
    return make_block([&] { return rr::make_channelizer(taps, nchan, ntaps, interp, deci, true); });
}
rr_block* rr_fm_receiver_create(const rr_c32* rf_taps, size_t nchan, size_t rf_ntaps, size_t rf_interp, size_t rf_deci, float gain,
                                int atan2_mode, const float* audio_taps, size_t audio_ntaps, size_t audio_interp, size_t audio_deci,
                                float scale) {
    return make_block([&] {
        return rr::make_fm_receiver(rf_taps, nchan, rf_ntaps, rf_interp, rf_deci, gain, atan2_mode, audio_taps, audio_ntaps,
                                    audio_interp, audio_deci, scale, false);
    });
}
rr_block* rr_fm_receiver_u8_create(const rr_c32* rf_taps, size_t nchan, size_t rf_ntaps, size_t rf_interp, size_t rf_deci, float gain,
                                   int atan2_mode, const float* audio_taps, size_t audio_ntaps, size_t audio_interp, size_t audio_deci,
                                   float scale) {
    return make_block([&] {
        return rr::make_fm_receiver(rf_taps, nchan, rf_ntaps, rf_interp, rf_deci, gain, atan2_mode, audio_taps, audio_ntaps,
                                    audio_interp, audio_deci, scale, true);
    });
}
size_t rr_block_out_windows(const rr_block* b) { return b ? b->b->out_windows() : 0; }
void rr_block_destroy(rr_block* b) { try { delete b; } catch (...) {} }

static int guarded(rr_block* b, size_t* consumed, size_t* produced, size_t* need, const char* what,
                   const std::function<int()>& f) {
    size_t dummy = 0;
    (void)dummy;
    if (!b || !consumed || !produced || !need) { rr::set_last_error(std::string(what) + ": null argument"); return RR_ERR; }
    try {
        return f();
    } catch (const std::exception& e) {
        rr::set_last_error(std::string(what) + ": " + e.what());
        *consumed = *produced = *need = 0;
        return RR_ERR;
    } catch (...) {
        rr::set_last_error("non-standard exception");
        *consumed = *produced = *need = 0;
        return RR_ERR;
    }
}

int rr_block_work(rr_block* b, const void* in, size_t in_len, void* out, size_t out_cap, size_t* consumed,
                  size_t* produced, size_t* need) {
    return guarded(b, consumed, produced, need, "rr_block_work",
                   [&] { return b->b->work_host(in, in_len, out, out_cap, consumed, produced, need); });
}
int rr_block_work_dev(rr_block* b, const void* d_in, size_t in_len, void* d_out, size_t out_cap, size_t* consumed,
                      size_t* produced, size_t* need, void* hip_stream) {
    return guarded(b, consumed, produced, need, "rr_block_work_dev", [&] {
        RR_HIP(hipSetDevice(b->b->device));
        // the handle is used as given: NULL is HIP's default stream (what torch's default stream is),
        // NOT the block's private stream — anything else would run unordered against the caller's work
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        b->b->last_stream = s;
        return b->b->work_dev(d_in, in_len, d_out, out_cap, consumed, produced, need, s);
    });
}
int rr_block_eof(rr_block* b, int src_eof) { return b && b->b->eof(src_eof != 0) ? 1 : 0; }
const char* rr_block_name(const rr_block* b) { return b ? b->b->name : ""; }
int rr_block_tag_rule(const rr_block* b, size_t* param) {
    if (!b) { rr::set_last_error("rr_block_tag_rule: null handle"); return RR_ERR; }
    if (param) *param = b->tag_param;
    return b->tag_rule;
}
size_t rr_block_in_elem_size(const rr_block* b) { return b ? b->b->in_es : 0; }
size_t rr_block_out_elem_size(const rr_block* b) { return b ? b->b->out_es : 0; }
int rr_block_sync(rr_block* b) {
    if (!b) return RR_ERR;
    try { b->b->sync(); return 0; } catch (const std::exception& e) { rr::set_last_error(e.what()); return RR_ERR; } catch (...) { rr::set_last_error("non-standard exception"); return RR_ERR; }
}

int rr_block_set_profiling(rr_block* b, int on) {
    if (!b) return RR_ERR;
    b->b->prof_on = on != 0;
    return 0;
}
int rr_block_profile(rr_block* b, double* total_ms, size_t* launches, int reset) {
    if (!b) return RR_ERR;
    try { RR_HIP(hipSetDevice(b->b->device)); b->b->prof_read(total_ms, launches, reset != 0); return 0; }
    catch (const std::exception& e) { rr::set_last_error(e.what()); return RR_ERR; } catch (...) { rr::set_last_error("non-standard exception"); return RR_ERR; }
}

unsigned long long rr_debug_kernel_launches(void) { return rr::g_kernel_launches.load(std::memory_order_relaxed); }
const char* rr_debug_last_kernel(const rr_block* b) { return b && b->b ? b->b->last_kernel : ""; }

/* measurement builds (make ABLATE=1): phase time stamps of one FftFilter tile; 0 in product builds */
int rr_debug_fft_stamps(unsigned long long* out16) {
    try { return rr::fft_read_stamps(out16); } catch (const std::exception& e) { rr::set_last_error(e.what()); return RR_ERR; } catch (...) { rr::set_last_error("non-standard exception"); return RR_ERR; }
}

int rr_fftfilter_dims(const rr_block* b, size_t* fft_size, size_t* nsamples, size_t* gpu_fft_size) {
    if (!b) return RR_ERR;
    const rr::FftFilter* f = dynamic_cast<const rr::FftFilter*>(b->b.get());
    if (!f) {
        if (auto* ff = dynamic_cast<const rr::FftFilterFloat*>(b->b.get())) f = ff->inner.get();
    }
    if (!f) { rr::set_last_error("rr_fftfilter_dims: not an FftFilter"); return RR_ERR; }
    if (fft_size) *fft_size = f->fft_size;
    if (nsamples) *nsamples = f->nsamples;
    if (gpu_fft_size) *gpu_fft_size = (size_t)1 << f->log2f;
    return 0;
}
size_t rr_fir_fft_tile(const rr_block* b) {
    if (!b) return 0;
    const rr::FirC32* f = dynamic_cast<const rr::FirC32*>(b->b.get());
    if (f && f->poly) return 1024;                            // decimate-first tiles: 1024 output-rate positions
    if (f && f->prune) return (size_t)1 << f->prune->log2f;
    if (f && f->half_ok) return 2048;
    return f && f->fftk ? (size_t)1 << f->fftk->log2f : 0;
}
// ---- host memory registration -----------------------------------------------------------------------
int rr_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) { rr::set_last_error("rr_host_register: null / empty range"); return RR_ERR; }
    return guarded([&] { RR_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault)); rr::host_range_add(ptr, bytes); });
}
int rr_host_window_in_place(const void* ptr, size_t bytes) { return ptr && bytes && rr::device_view_of_host(ptr, bytes) ? 1 : 0; }
int rr_host_unregister(void* ptr) {
    if (!ptr) { rr::set_last_error("rr_host_unregister: null"); return RR_ERR; }
    return guarded([&] { rr::host_range_remove(ptr); RR_HIP(hipHostUnregister(ptr)); });
}

// ---- device-resident streams ------------------------------------------------------------------------
rr_dstream* rr_dstream_create(size_t elem_size, size_t capacity_bytes) {
    rr::OptsScope scope;
    try {
        static std::atomic<size_t> next_id{1};
        std::unique_ptr<rr::DStream> d(new rr::DStream(elem_size, capacity_bytes));
        auto* h = new rr_dstream;
        h->s = std::move(d);
        h->id = next_id++;
        return h;
    } catch (const std::exception& e) {
        rr::set_last_error(e.what());
        return nullptr;
    } catch (...) {
        rr::set_last_error("non-standard exception");
        return nullptr;
    }
}
void rr_dstream_destroy(rr_dstream* s) { try { delete s; } catch (...) {} }
size_t rr_dstream_capacity(const rr_dstream* s) { return s ? s->s->cap : 0; }
int rr_dstream_is_double_mapped(const rr_dstream* s) { return s && s->s->vmm ? 1 : 0; }
size_t rr_dstream_id(const rr_dstream* s) { return s ? s->id : 0; }
size_t rr_dstream_read_buf(rr_dstream* s, const void** dev_ptr) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(s->m);
    if (dev_ptr) *dev_ptr = s->s->read_ptr();
    return s->s->used();
}
size_t rr_dstream_write_buf(rr_dstream* s, void** dev_ptr, void* hip_stream) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(s->m);
    try {
        if (!dev_ptr) return s->s->free();         // a count only: nothing is about to be written
        RR_HIP(hipSetDevice(s->s->device));        // write_ptr may enqueue the fallback ring's move
        s->s->will_write(static_cast<hipStream_t>(hip_stream));   // the caller writes the window on this stream
        *dev_ptr = s->s->write_ptr(static_cast<hipStream_t>(hip_stream));
        return s->s->free();
    } catch (const std::exception& e) {
        rr::set_last_error(e.what());
        return 0;
    } catch (...) {
        rr::set_last_error("non-standard exception");
        return 0;
    }
}
int rr_dstream_consume(rr_dstream* s, size_t n) {
    if (!s) { rr::set_last_error("null dstream"); return RR_ERR; }
    std::lock_guard<std::mutex> g(s->m);
    const int rc = guarded([&] { s->s->consume(n); });
    if (n) s->cv.notify_all();
    return rc;
}
int rr_dstream_produce(rr_dstream* s, size_t n) {
    if (!s) { rr::set_last_error("null dstream"); return RR_ERR; }
    std::lock_guard<std::mutex> g(s->m);
    const int rc = guarded([&] { s->s->produce(n); });
    if (n) s->cv.notify_all();
    return rc;
}
int rr_dstream_close(rr_dstream* s, int side) {
    if (!s || (side != RR_SIDE_WRITER && side != RR_SIDE_READER)) { rr::set_last_error("rr_dstream_close: bad argument"); return RR_ERR; }
    std::lock_guard<std::mutex> g(s->m);
    s->closed[side] = true;
    s->cv.notify_all();
    return 0;
}
int rr_dstream_closed(rr_dstream* s, int side) {
    if (!s || (side != RR_SIDE_WRITER && side != RR_SIDE_READER)) return 1;
    std::lock_guard<std::mutex> g(s->m);
    return s->closed[side] ? 1 : 0;
}
size_t rr_dstream_wait(rr_dstream* s, int side, size_t need, unsigned timeout_ms, int* never) {
    if (never) *never = 1;
    if (!s || (side != RR_SIDE_WRITER && side != RR_SIDE_READER)) return 0;
    std::unique_lock<std::mutex> g(s->m);
    // the READER waits for samples and gives up when the writer is gone; the WRITER waits for room and gives up when
    // the reader is gone (ReadStream::wait_for_read / WriteStream::wait_for_write, src/stream.rs:222-224,311-313)
    const int other = side == RR_SIDE_READER ? RR_SIDE_WRITER : RR_SIDE_READER;
    auto have = [&] { return side == RR_SIDE_READER ? s->s->used() : s->s->free(); };
    s->cv.wait_for(g, std::chrono::milliseconds(timeout_ms), [&] { return have() >= need || s->closed[other]; });
    const size_t n = have();
    if (never) *never = (n < need && s->closed[other]) ? 1 : 0;
    return n;
}
int rr_dstream_copy_in(rr_dstream* s, size_t offset, const void* host, size_t n, void* hip_stream) {
    if (!s) { rr::set_last_error("null dstream"); return RR_ERR; }
    auto st = static_cast<hipStream_t>(hip_stream);
    int rc;
    {
        std::lock_guard<std::mutex> g(s->m);
        rc = guarded([&] {
            rr::DStream& d = *s->s;
            RR_HIP(hipSetDevice(d.device));
            d.will_write(st);
            unsigned char* w = static_cast<unsigned char*>(d.write_ptr(st));
            if (offset + n > d.free()) throw rr::Error("dstream copy_in: beyond the write window");
            // a window of a ring the shim registered (zero-copy admitted): a copy kernel reads it in place over PCIe, 3x the
            // rate hipMemcpyAsync gets out of such a range on this platform (kernels_misc.hip launch_copy_bytes)
            void* hv = n ? rr::device_view_of_host(host, n * d.es) : nullptr;
            if (hv) rr::launch_copy_bytes(hv, w + offset * d.es, n * d.es, st);
            else if (n && rr::host_range_registered(host, n * d.es)) RR_HIP(hipMemcpyAsync(w + offset * d.es, host, n * d.es, hipMemcpyHostToDevice, st));
            else if (n) rr::stage_upload_sync(w + offset * d.es, host, n * d.es, st);     // pageable: stage.hpp
        });
    }
    if (rc != 0 || n == 0) return rc;
    // `host` is the caller's to reuse on return: a source ring's window is consumed right after this call and its writer
    // overwrites it.  From pageable memory the runtime has already staged the bytes; from a page-locked (rr_host_register'd)
    // ring the DMA is still reading, so wait for it -- outside the lock, the reader may go on consuming meanwhile.
    return guarded([&] { RR_HIP(hipStreamSynchronize(st)); });
}
int rr_dstream_copy_out(rr_dstream* s, size_t offset, void* host, size_t n, void* hip_stream) {
    if (!s) { rr::set_last_error("null dstream"); return RR_ERR; }
    auto st = static_cast<hipStream_t>(hip_stream);
    int rc;
    {
        std::lock_guard<std::mutex> g(s->m);
        rc = guarded([&] {
            rr::DStream& d = *s->s;
            if (offset + n > d.used()) throw rr::Error("dstream copy_out: beyond the read window");
            RR_HIP(hipSetDevice(d.device));
            d.will_read(st);
            void* hv = n ? rr::device_view_of_host(host, n * d.es) : nullptr;
            const unsigned char* rp = static_cast<const unsigned char*>(d.read_ptr()) + offset * d.es;
            if (hv) rr::launch_copy_bytes(rp, hv, n * d.es, st);              // (see copy_in)
            else if (n && rr::host_range_registered(host, n * d.es)) RR_HIP(hipMemcpyAsync(host, rp, n * d.es, hipMemcpyDeviceToHost, st));
            else if (n) rr::stage_download_sync(host, rp, n * d.es, st);                   // pageable: stage.hpp
        });
    }
    if (rc != 0) return rc;
    // outside the lock: the writer may go on filling the free space while this window crosses the bus (the read window
    // is not released before the caller's rr_dstream_consume)
    return guarded([&] { RR_HIP(hipStreamSynchronize(st)); });          // the host may read `host` on return
}
int rr_dstream_copy(rr_dstream* dst, size_t dst_offset, rr_dstream* src, size_t src_offset, size_t n, void* hip_stream) {
    if (!dst || !src || dst == src) { rr::set_last_error("rr_dstream_copy: null dstream / same ring on both sides"); return RR_ERR; }
    std::scoped_lock g(src->m, dst->m);
    return guarded([&] {
        rr::DStream& d = *dst->s;
        rr::DStream& r = *src->s;
        auto st = static_cast<hipStream_t>(hip_stream);
        if (d.es != r.es) throw rr::Error("dstream copy: element sizes differ");
        if (d.device != r.device) throw rr::Error("dstream copy: rings on different devices");
        if (src_offset + n > r.used()) throw rr::Error("dstream copy: beyond the read window");
        RR_HIP(hipSetDevice(d.device));
        r.will_read(st);
        d.will_write(st);
        unsigned char* w = static_cast<unsigned char*>(d.write_ptr(st));
        if (dst_offset + n > d.free()) throw rr::Error("dstream copy: beyond the write window");
        if (n) RR_HIP(hipMemcpyAsync(w + dst_offset * d.es, static_cast<const unsigned char*>(r.read_ptr()) + src_offset * r.es, n * d.es,
                                     hipMemcpyDeviceToDevice, st));
    });
}
int rr_block_work_streams(rr_block* b, rr_dstream* src, rr_dstream* dst, size_t* consumed, size_t* produced,
                          size_t* need, void* hip_stream) {
    size_t c = 0, p = 0, nd = 0;
    if (!b || !src || !dst || src == dst) { rr::set_last_error("rr_block_work_streams: null argument / same ring on both sides"); return RR_ERR; }
    if (b->b->out_windows() != 1) { rr::set_last_error("rr_block_work_streams: single-output blocks only"); return RR_ERR; }
    if (src->s->es != b->b->in_es || dst->s->es != b->b->out_es) {
        rr::set_last_error("rr_block_work_streams: stream element size does not match the block");
        return RR_ERR;
    }
    int st = RR_ERR;
    // both rings for the whole call: windows, enqueue and the consume / produce are one step to every other thread
    std::scoped_lock g(src->m, dst->m);
    const int rc = guarded([&] {
        auto hs = static_cast<hipStream_t>(hip_stream);
        RR_HIP(hipSetDevice(dst->s->device));
        src->s->will_read(hs);
        dst->s->will_write(hs);
        void* out = dst->s->write_ptr(hs);
        st = rr_block_work_dev(b, src->s->read_ptr(), src->s->used(), out, dst->s->free(), &c, &p, &nd, hip_stream);
        if (st == RR_ERR) return;
        src->s->consume(c);
        dst->s->produce(p);
    });
    if (c) src->cv.notify_all();
    if (p) dst->cv.notify_all();
    if (consumed) *consumed = c;
    if (produced) *produced = p;
    if (need) *need = nd;
    return rc == 0 ? st : RR_ERR;
}

int rr_fir_set_rotator_mode(rr_block* b, int mode) {
    auto* f = b ? dynamic_cast<rr::FirC32*>(b->b.get()) : nullptr;
    if (!f && b) if (auto* hf = dynamic_cast<rr::HilbertFir*>(b->b.get())) f = hf->fir.get();
    if (!f || (mode != RR_ROT_MODEL && mode != RR_ROT_REPLAY && mode != RR_ROT_REPLAY_DEVICE && mode != RR_ROT_REPLAY_HOST)) { rr::set_last_error("rr_fir_set_rotator_mode: bad argument"); return RR_ERR; }
    f->rot_mode = mode;
    return 0;
}

}  // extern "C"
