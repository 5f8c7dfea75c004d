// blocks_packet.hpp — the packet-side blocks (blocks_packet.cpp) and the plumbing they share.  Part of blocks.hpp: include that.
#pragma once
#include "blocks.hpp"
#include "hdlcrx_host.hpp"
#include "il2p_host.hpp"
#include "pwm_host.hpp"
#include "afsk_host.hpp"
#include "am_host.hpp"
#include "fsk_host.hpp"
#include "kiss_host.hpp"

namespace rr {

// What a block carries from call to call on the device, as a pair: a call reads in() and writes out(), then flip()s, so a call
// that is still in flight on another stream never has its input overwritten.
template <class T> struct Carried {
    DevBuf<T> buf[2];
    int cur = 0;
    T* in() const { return buf[cur].p; }
    T* out() const { return buf[cur ^ 1].p; }
    void flip() { cur ^= 1; }
    void reserve_out(size_t n) { buf[cur ^ 1].reserve(n); }
    void zero(size_t n, hipStream_t s) { for (auto& b : buf) { b.reserve(n); RR_HIP(hipMemsetAsync(b.p, 0, n * sizeof(T), s)); } }
    void upload(const T* h, size_t n, hipStream_t s) { for (auto& b : buf) b.upload(h, n, s); }
};

// The list a call left on the device, count first: refused with `msg` beyond `cap` entries.  list(k) says where the k > 0
// entries are (BitDecoder packs them only once it knows k).
template <class H, class F>
void fetch_counted_at(const unsigned long long* d_count, F&& list, size_t cap, const char* msg, std::vector<H>& dst, hipStream_t s) {
    unsigned long long k = 0;
    stage_download_sync(&k, d_count, sizeof k, s);
    if (k > cap) throw Error(msg);
    dst.resize((size_t)k);
    if (k) stage_download_sync(dst.data(), list((size_t)k), (size_t)k * sizeof(H), s);
}
template <class H, class D>
void fetch_counted(const unsigned long long* d_count, const D* d_list, size_t cap, const char* msg, std::vector<H>& dst, hipStream_t s) {
    static_assert(sizeof(D) == sizeof(H), "the device's entry is the host's");
    fetch_counted_at(d_count, [&](size_t) { return d_list; }, cap, msg, dst, s);
}

// #[rustradio(sync)] blocks (rustradio_macros_code/src/lib.rs:458-515): map min(input, output space) samples,
// then WaitForStream on the side that ran dry.
struct SyncBlock : Block {
    using Block::Block;
    int work_dev(const void*, size_t, void*, size_t, size_t*, size_t*, size_t*, hipStream_t) final;
protected:
    virtual void begin_call() {}          // every call, also one that moves nothing (the blocks that keep a per-call list drop it here)
    virtual void run(const void* in, void* out, size_t n, hipStream_t s) = 0;     // n > 0, inside the profiling bracket
};
struct MultiplyConst : SyncBlock {        // multiply_const.rs:6-23, T = Float (es 4) or Complex (es 8)
    float vr, vi;
    MultiplyConst(size_t es, float re, float im);
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
struct AddConst : SyncBlock {             // add_const.rs:51-68, T = Float (es 4) or Complex (es 8): one f32 add per component
    float vr, vi;
    AddConst(size_t es, float re, float im);
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
struct FastFM : SyncBlock {           // quadrature_demod.rs:144-165; q2, q1 = the two previous samples (zeros at start)
    Carried<cf> hist;
    FastFM();
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
// Vco (vco.rs:9-37): Float -> Complex(sin phase, cos phase), phase += k * a in f64.  The running sum is a tiled scan
// (kernels_tx.hip); the phase carried from call to call stays on the device — the host never reads it, counts depend on lengths only.
struct VcoState {
    double k;
    Carried<double> phase;            // in(): the phase after the last sample of the previous call (0 at start)
    DevBuf<double> tiles;             // scan scratch: one double per tile of the largest window so far
    VcoState(double k, hipStream_t s);
    double* scratch(size_t n) { tiles.reserve((n + VCO_T - 1) / VCO_T); return tiles.p; }
};
struct Vco : SyncBlock {
    VcoState v;
    explicit Vco(double k);
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
// RationalResampler::new(src, interp, deci) -> Vco::new(_, k) fused (examples/fm_tx.rs:84-91): f32 in, Complex out.  The window
// protocol, `pending` and eof are the resampler's own code; the interpolated f32 stream exists only as the scan's index map.
struct FmTx : Resampler {
    VcoState v;
    FmTx(size_t interp, size_t deci, double k);
protected:
    void emit(const void* in, void* out, int64_t r, int64_t n_gather, int64_t c0, hipStream_t s) override;
};

// ComplexToMag2 (complex_to_mag2.rs:8-21): Complex -> re * re + im * im, a sync block.  Bit-exact.
struct ComplexToMag2 : SyncBlock {
    ComplexToMag2();
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
// The first Map of examples/airspy_am_decode.rs ("AirSPY to Complex"): u32 (i16 I low, i16 Q high) -> Complex(i / 1000, q / 1000),
// a sync block.  Bit-exact.
struct AirspyDecode : SyncBlock {
    AirspyDecode();
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
// SinglePoleIirFilter (single_pole_iir_filter.rs:11-93): y = alpha x + fl32(1 - alpha) y_prev as a tiled f64 scan
// (kernels_burst.hip).  y_prev stays on the device, one f64 per row (Complex: re, im); the host never reads it.
struct IirState {
    IirCoef c{};
    DevBuf<double> pw8, pws;          // the powers of b the scan combines runs with
    Carried<double> y;                // in(): y after the last sample of the previous call (0 at start)
    int rows = 1;
    DevBuf<double> tiles;             // scan scratch: one double per row and tile of the largest window so far
    IirState(float alpha, int rows, hipStream_t s);    // throws "alpha out of range" unless 0 <= alpha <= 1
    double* scratch(size_t n) { tiles.reserve((size_t)rows * ((n + IIR_T - 1) / IIR_T)); return tiles.p; }
};
struct SinglePoleIir : SyncBlock {
    IirState st;
    SinglePoleIir(float alpha, size_t es);
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};
// ComplexToMag2 -> SinglePoleIirFilter(alpha) -> the comparison of BurstTagger(threshold) (burst_tagger.rs:68-85) fused
// (examples/burst_saver.rs:111-123): Complex in, the filtered power out, and per call the list of threshold crossings.
struct BurstDetector : SyncBlock {
    IirState st;
    float thr;
    Carried<int> flag;                        // in(): out > threshold at the last sample of the previous call (false at start)
    Carried<unsigned long long> count;        // in(): entries of the most recent call's list
    DevBuf<unsigned long long> list;          // (pos << 1) | cur, unordered; one slot per sample of the largest window so far
    bool fetched = true;                      // `edges` holds the most recent call's list
    std::vector<unsigned long long> edges;    // ... ascending
    BurstDetector(float alpha, float threshold);
    void begin_call() override;
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
    const std::vector<unsigned long long>& fetch_edges();   // waits for the most recent call
};

// The bit-level sync blocks (kernels_bits.hip): BinarySlicer (binary_slicer.rs:17-19), XorConst(1), NrziDecode
// (nrzi.rs:36-41), Descrambler (descrambler.rs:34-39), CorrelateAccessCodeTag (correlate_access_code.rs:93-118) — any subset,
// in that order, as ONE kernel.  f32 in (the slicer is then the first stage) or u8 in; u8 out.  The state between calls
// (BITS_ST_*) stays on the device; the host reads only the tag list, and only when asked.
struct BitDecoder : SyncBlock {
    BitsCfg cfg{};
    Carried<unsigned long long> st;           // in(): what the stream so far left behind
    DevBuf<unsigned> tilecnt;                 // tags of every tile of the most recent call
    DevBuf<unsigned long long> list;          // (pos << 8) | diffs: tile t's at [t BITS_T ..), BITS_T slots each; grows with the window
    DevBuf<unsigned long long> offs, total, packed;   // rr_bit_tags: the entries before each tile, their sum, the list without gaps
    size_t last_tiles = 0;                    // tiles of the most recent call
    bool fetched = true;                      // `tags` holds the most recent call's list
    std::vector<unsigned long long> tags;     // ... ascending
    // f32src: the slicer in front.  code_len == 0: no correlator.  Throws on the parameter errors of bits_check().
    BitDecoder(const char* nm, bool f32src, int flags, unsigned long long mask, unsigned long long seed, unsigned len,
               unsigned long long code, unsigned code_len, size_t allowed_diffs);
    bool has_correlator() const { return cfg.L != 0; }
    void begin_call() override;
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
    const std::vector<unsigned long long>& fetch_tags();    // waits for the most recent call
};
// nullptr, or what is wrong with the parameters (said before any device is touched)
const char* bits_check(int flags, unsigned long long seed, unsigned len, unsigned code_len);

// The handles with no stream protocol: work_dev only throws `no_stream`.
struct BatchBlock : Block {
    const char* no_stream;
    BatchBlock(const char* nm, size_t ies, size_t oes, const char* sentence) : Block(nm, ies, oes), no_stream(sentence) {}
    int work_dev(const void*, size_t, void*, size_t, size_t*, size_t*, size_t*, hipStream_t) final { throw Error(no_stream); }
protected:
    // a call on host buffers: the body runs on the handle's own stream and has completed on return
    template <class F> void host_call(F&& body) {
        RR_HIP(hipSetDevice(device));
        last_stream = stream;
        body();
        RR_HIP(hipStreamSynchronize(stream));
        hstage().quiesced();
    }
    void settle() { sync(); if (hstage_) hstage_->quiesced(); }      // in front of every fetch: the latest call has completed
};

// Wpcr (wpcr.rs:105-239) in PDU form over a batch of disjoint bursts of one f32 buffer (kernels_wpcr.hip): no stream protocol
// (work_dev is an error), no state between calls.  The scratch buffers are as long as the largest sample buffer so far and a
// burst owns the range of each that its samples have in the input; the host keeps only the geometry of the latest call.
struct Wpcr : BatchBlock {
    static constexpr size_t MAX_LEN = 512000;     // the reference's stream capacity in f32 samples (stream.rs:105)
    float samp_rate;                              // NaN: not set
    DevBuf<unsigned> list, tilecnt;               // crossing positions (burst-owned slots); crossings of every sample tile
    DevBuf<float> mag, reim;                      // |X[k]| and Re X / Im X of every burst's bins
    DevBuf<unsigned char> desc;                   // this call's WpcrBurst records and the two tile -> burst maps
    DevBuf<WpcrResult> res;
    DevBuf<float> h_in, h_out;                    // process(): the host buffers' device copies
    std::vector<unsigned char> hdesc;
    std::vector<size_t> starts, lens;             // the latest call's geometry
    bool fetched = true;                          // `results` holds the latest call's records
    std::vector<WpcrResult> results;
    explicit Wpcr(float samp_rate);
    // throws "bursts overlap" / "burst outside the buffer" / "burst longer than 512000 samples"; the process calls run it before
    // anything is enqueued
    static void check(size_t n_total, const size_t* st, const size_t* ln, size_t nbursts);
    void process_dev(const float* d_x, size_t n_total, const size_t* st, const size_t* ln, const float* mid, size_t nbursts,
                     float* d_syms, hipStream_t s);
    void process_host(const float* x, size_t n_total, const size_t* st, const size_t* ln, const float* mid, size_t nbursts,
                      float* syms);
    const std::vector<WpcrResult>& fetch_results();          // waits for the latest call
    std::vector<float> fetch_spectrum(size_t burst);         // ... and downloads mag[0 .. N / 2) of one of its bursts
    // PduToStream over the latest call (rr_wpcr_pack_dev): waits for its results, then one gather launch on s
    DevBuf<long> pack_desc;
    std::vector<long> hpack;
    void pack_dev(const float* d_syms, float* d_out, size_t out_cap, size_t* produced, size_t* pdu_start, size_t* pdu_len, size_t cap,
                  size_t* npdus, hipStream_t s);
};

// BurstTagger -> StreamToPdu -> [Midpointer] over windows of a data / f32 trigger stream pair (kernels_pdu.hip): no stream
// protocol (work_dev is an error).  The data is f32 (es 4) or Complex (es 8: no Midpointer, which is a block over Vec<Float>).
// The state between pushes (PduState) stays on the device; the two arenas alternate, and the one of the previous push holds the
// samples of a burst that is still open, so they are the carry as well.
struct StreamToPdu : BatchBlock {
    static constexpr size_t MAX_WINDOW = 1024000;         // the f32 stream capacity in samples (stream.rs:105)
    float thr;
    size_t max_size, tail;
    bool midpoint;
    size_t es;                                    // bytes of a data sample: 4 or 8
    Carried<PduState> st;
    Carried<float> arena;                         // in(): the arena of the most recent push that moved samples (es / 4 floats a sample)
    size_t n_prev = 0, n_total = 0;               // its window; its length in samples (0: no such push yet, or the latest push was empty)
    unsigned long long w0 = 0;                    // samples of the stream so far
    DevBuf<unsigned> tilecnt, edges, jmp[2], mark;
    DevBuf<unsigned long long> offs, etotal, count;
    DevBuf<PduRoot> root;
    DevBuf<PduRec> recs;
    DevBuf<float> ranks;                          // Midpointer's low and high per record slot (rr_debug_pdu_ranks)
    DevBuf<float> h_data, h_trig;                 // push(): the host windows' device copies
    size_t last_n = 0;                            // the most recent push's window
    bool fetched = true, efetched = true;         // `records` / `edgelist` hold the most recent push's
    std::vector<rr_pdu_record> records;           // ... ascending
    std::vector<size_t> slots;                    // record i's place in the device's (unordered) list
    std::vector<unsigned> edgelist;               // (pos << 1) | cur, ascending
    StreamToPdu(float threshold, size_t max_size, size_t tail, int flags, size_t es = 4);
    void push_dev(const void* d_data, const float* d_trig, size_t n, hipStream_t s);
    void push_host(const void* data, const float* trig, size_t n);
    const std::vector<rr_pdu_record>& fetch_records();      // waits for the most recent push
    const std::vector<unsigned>& fetch_edges();
    const void* arena_dev() const { return n_total ? arena.in() : nullptr; }
    void fetch_pdu(size_t idx, void* out, size_t cap);      // cap in samples
    void fetch_ranks(size_t idx, float* low, float* high);  // the two elements Midpointer's offset of PDU idx was made of
protected:
    StreamToPdu(const char* nm, const char* sentence, float threshold, size_t max_size, size_t tail, int flags, size_t es);
    // the three parts of a push of n <= MAX_WINDOW samples: drop the previous push's results and size the buffers (false: n == 0,
    // nothing to do); what the kernels get; the flips once everything is enqueued
    bool begin_push(size_t n);
    PduArgs push_args(const void* d_data, const float* d_trig, size_t n);
    void end_push(size_t n);
};

// Delay<T> (src/delay.rs:62-111) for elements of 1, 4 or 8 bytes: `delay` default elements, then the input.  What is left of the
// delay is host state; a call moves min(remaining, out_cap) zeros and then min(in_len, the space left) samples in one launch.
struct Delay : Block {
    size_t delay, remaining;
    Delay(size_t delay, size_t es);
    int work_dev(const void* in, size_t in_len, void* out, size_t out_cap, size_t* consumed, size_t* produced, size_t* need,
                 hipStream_t s) override;
    bool eof(bool src_eof) override { return src_eof && remaining == 0; }        // delay.rs:56-60
};

// examples/burst_saver.rs:111-131 behind one handle: [ComplexToMag2 -> SinglePoleIirFilter] and [Delay] on the two branches of
// the Tee, BurstTagger -> StreamToPdu<Complex> behind them.  A StreamToPdu whose trigger is made here (the detector's scan) and
// whose arena is filled by k_saver_copy from the window and the history: the last `delay` input samples, a ping-pong pair.
struct BurstSaver : StreamToPdu {
    IirState iir;
    size_t delay;
    Carried<unsigned long long> hist;             // in(): the last `delay` input samples (zeros in front of the stream)
    DevBuf<float> env;                            // the envelope, when the caller does not want it
    DevBuf<cf> h_in;                              // push(): the host window's device copy
    DevBuf<float> h_env;
    BurstSaver(float alpha, float threshold, size_t delay, size_t max_size, size_t tail);
    void push_dev(const cf* d_in, size_t n, float* d_env, hipStream_t s);
    void push_host(const cf* in, size_t n, float* env);
};

// Scrambler::g3ruh (descrambler.rs:41-47, 95-123) and NrziEncode (nrzi.rs:52-69) as one affine system over GF(2)
// (kernels_frame.hip, frame_core.hpp): what LineCoder (the two sync blocks) and HdlcFramer share.  The state word stays on the
// device between calls; mode 0 has none.
struct LineState {
    int mode = 0;                             // LINE_SCR | LINE_NRZI
    DevBuf<unsigned> pw;                      // the LINE_NP powers of the tile matrix
    Carried<unsigned> st;                     // in(): what the stream so far left behind
    DevBuf<unsigned> z, carry;                // one word per tile of the largest call so far
    void init(int mode, hipStream_t s);
    // n = *n_dev when given (at most max_n), else max_n
    void run(const unsigned char* in, void* out, bool out_f32, float lo, float hi, size_t max_n, const unsigned long long* n_dev,
             hipStream_t s);
};
struct LineCoder : SyncBlock {
    LineState line;
    LineCoder(const char* nm, int mode);
    void run(const void* in, void* out, size_t n, hipStream_t s) override;
};

// FcsAdder -> HdlcFramer -> PduToStream<u8> -> [Scrambler::g3ruh] -> [NrziEncode] -> [Map] in PDU form over a batch of packets of
// one byte buffer (kernels_frame.hip): no stream protocol (work_dev is an error).  The host keeps the geometry of the latest
// push; what it reads back (frame_host.hpp) is sized from that geometry.
struct HdlcFramer : BatchBlock {
    int flags;
    float lo, hi;
    LineState line;
    DevBuf<unsigned long long> desc, total;   // this push's starts / pb / cpre; the framed bits it made
    DevBuf<unsigned> part, crc, sums, tin, cb;
    DevBuf<unsigned char> lb, pre;            // the packets' bytes with their FCS; the framed bits in front of the line coder
    DevBuf<unsigned char> h_in, h_out;        // push_host(): the host buffers' device copies
    std::vector<size_t> lens;                 // the latest push's geometry
    size_t bound = 0;
    bool fetched = true;                      // `records` / `produced` hold the latest push's
    std::vector<rr_frame_record> records;
    size_t produced = 0;
    HdlcFramer(int flags, float lo, float hi);
    void push_dev(const unsigned char* d_bytes, size_t n_bytes, const size_t* starts, const size_t* lens, size_t npackets, void* d_out,
                  size_t out_cap, hipStream_t s);
    void push_host(const unsigned char* bytes, size_t n_bytes, const size_t* starts, const size_t* lens, size_t npackets, void* out,
                   size_t out_cap, size_t* produced);
    const std::vector<rr_frame_record>& fetch_records();      // waits for the latest push
};

// What rr_hdlc_deframer and rr_hdlc_receiver share on the host: nstreams HdlcDeframers' state between pushes (per stream the
// machine at the last flag end, the counters and the raw bits of the gap still open, all on the device), the workspace of a push
// and the read-back.  Not a Block: both handles hold one, the deframer's with nstreams == 1.  The host keeps ONE upper bound of
// the carried bits for all streams; hdlc_plan (hdlc_host.hpp) turns it and a push's length into every size here.
struct HdlcCore {
    size_t nstreams = 1, min_size = 0, max_size = 0;
    int flags = 0;                                // RR_HDLC_*
    Carried<HdlcState> st;                        // in(): what the streams so far left behind, one per stream
    Carried<unsigned char> cbits;                 // ... and its carried bits, one per byte: hdlc_carry_bits(max_size) per stream
    size_t carry = 0;                             // the carried bits of any stream, at most
    DevBuf<unsigned long long> raw, fl, ab, sf, offs, etotal, pstats, count;
    DevBuf<unsigned> tilecnt, ends;
    DevBuf<unsigned char> gmap, pmap, bmap, bstate, arena;
    DevBuf<int> fin;
    size_t last_n = 0, last_carry = 0;            // the most recent push: its bits per stream, at most; the carry bound it began with
    bool bfetched = true;                         // `bytes` holds the most recent push's
    std::vector<unsigned char> bytes;
    // Unsynced(0xff) in front of every stream; the caller waits for s
    void init(size_t nstreams, size_t min_size, size_t max_size, int flags, hipStream_t s);
    // every push, also one of nothing: it has no bytes and leaves every state alone
    void begin(size_t n) { bytes.clear(); bfetched = true; last_n = n; }
    // n > 0: reserves the workspace, fills stream 0's view (all of HdlcArgs but bits, n, w0 and recs) and the pitches of the
    // others (rx may be null) -> the bounds of the push
    HdlcRxBounds plan(size_t n, HdlcArgs& a, HdlcRxArgs* rx);
    void advance(size_t n);                       // behind the launches: the out halves are what the next push starts from
    HdlcRxBounds bounds() const { return hdlcrx_bounds(nstreams, last_carry, last_n); }      // of the most recent push
    // The read-back of a push the caller has waited for, one download each (`count` is read by the handle, in front of its
    // records).  The counters of every stream's HdlcState, 3 per stream; before: the pair's other half, what the push started from
    std::vector<unsigned long long> fetch_stats(bool before, hipStream_t s) const;
    const std::vector<unsigned char>& fetch_bytes(hipStream_t s);             // only behind a push whose records stood the checks
    size_t arena_len() const { return last_n ? bounds().arena : 0; }
    const unsigned char* arena_dev() const { return arena_len() ? arena.p : nullptr; }
};

// HdlcDeframer (hdlc_deframer.rs:80-232) over windows of a bit stream (kernels_hdlc.hip): no stream protocol (work_dev is an
// error).  The one-stream case of HdlcCore; the handle's own are the stream position, the byte source and the rr_hdlc_frame records.
struct HdlcDeframer : BatchBlock {
    HdlcCore core;
    unsigned long long w0 = 0;                    // bits of the stream so far
    DevBuf<HdlcRec> recs;
    DevBuf<unsigned char> h_bits;                 // push_host(): the host window's device copy
    bool fetched = true;                          // `frames` holds the most recent push's
    std::vector<rr_hdlc_frame> frames;           // ... ascending by pos
    HdlcDeframer(size_t min_size, size_t max_size, int flags);
    void push_dev(const unsigned char* d_bits, size_t n, hipStream_t s);
    void push_host(const unsigned char* bits, size_t n);
    const std::vector<rr_hdlc_frame>& fetch_frames();         // waits for the most recent push
    const std::vector<unsigned char>& fetch_bytes();
    void fetch_stats(unsigned long long out[3]);
};

// KissFrame -> KissDecode (kiss.rs:96-228) over windows of a byte stream (kernels_kiss.hip): no stream protocol (work_dev is an
// error).  Everything between pushes (KissState: synced or not, the counters; the open gap's bytes) stays on the device in pairs;
// the host keeps the stream position and ONE upper bound of the carried bytes, which with a push's length gives every size here.
struct KissDecode : BatchBlock {
    size_t max_len;
    Carried<KissState> st;                        // in(): what the stream so far left behind
    Carried<unsigned char> cbytes;                // ... and the bytes of its open gap: max_len each
    size_t carry = 0;                             // the carried bytes, at most
    unsigned long long w0 = 0;                    // bytes of the stream so far
    DevBuf<unsigned> sums, tin, root, tsum, toff, obase;
    DevBuf<unsigned long long> count;
    DevBuf<unsigned char> arena;
    DevBuf<KissRec> recs;
    DevBuf<unsigned char> h_bytes;                // push_host(): the host window's device copy
    size_t last_n = 0, last_carry = 0;            // the most recent push: its bytes; the carry bound it began with
    bool fetched = true, bfetched = true;         // `packets` / `bytes` hold the most recent push's
    std::vector<rr_kiss_packet> packets;          // ... ascending by pos
    std::vector<unsigned char> bytes;
    explicit KissDecode(size_t max_len);
    void push_dev(const unsigned char* d_bytes, size_t n, hipStream_t s);
    void push_host(const unsigned char* bytes, size_t n);
    const std::vector<rr_kiss_packet>& fetch_packets();       // waits for the most recent push
    const std::vector<unsigned char>& fetch_bytes();
    void fetch_stats(unsigned long long out[5]);
    size_t arena_len() const { return last_n ? kiss_plan(last_carry, last_n).arena_cap : 0; }
    const unsigned char* arena_dev() const { return arena_len() ? arena.p : nullptr; }
};

// KissEncode -> PduToStream<u8> (kiss.rs:247-286) in PDU form over a batch of packets of one byte buffer (kernels_kiss.hip): no
// stream protocol (work_dev is an error), no state between pushes.  The host keeps the geometry of the latest push; what it
// reads back (kiss_host.hpp) is sized from that geometry.
struct KissEncode : BatchBlock {
    DevBuf<unsigned long long> desc, total;       // this push's starts / pb / ports; the bytes it made
    DevBuf<unsigned> tcnt, tin, cb;
    DevBuf<unsigned char> h_in, h_out;            // push_host(): the host buffers' device copies
    std::vector<size_t> lens;                     // the latest push's geometry
    std::vector<unsigned> ports;
    size_t bound = 0;
    bool fetched = true;                          // `records` / `produced` hold the latest push's
    std::vector<rr_kiss_frame_record> records;
    size_t produced = 0;
    KissEncode();
    void push_dev(const unsigned char* d_bytes, size_t n_bytes, const size_t* starts, const size_t* lens, const unsigned* ports,
                  size_t npackets, void* d_out, size_t out_cap, hipStream_t s);
    void push_host(const unsigned char* bytes, size_t n_bytes, const size_t* starts, const size_t* lens, const unsigned* ports,
                   size_t npackets, unsigned char* out, size_t out_cap, size_t* produced);
    const std::vector<rr_kiss_frame_record>& fetch_records();     // waits for the latest push
};

// [ComplexToMag2 ->] PwmDecoder (pwm_decoder.rs:385-513) over windows of a power or Complex stream (kernels_pwm.hip): no stream
// protocol (work_dev is an error).  Everything between pushes (PwmState, the open frame's bits, the candidate table) stays on the
// device in pairs; the host keeps the stream position, which bounds first_sample, and the plan of the most recent push.
struct PwmDecoder : BatchBlock {
    PwmCfg cfg{};
    size_t pitch;                                 // bytes of a candidate row
    Carried<PwmState> st;                         // in(): what the stream so far left behind
    Carried<unsigned char> fbits, cand;           // ... the open frame's bits; the candidates' bits
    Carried<PwmCand> meta;                        // ... and their numbers
    DevBuf<unsigned short> cls;
    DevBuf<unsigned char> tmap, tstate, ebits, arena;
    DevBuf<unsigned> tilecnt, offs, edges;
    DevBuf<unsigned long long> etotal, count;
    DevBuf<PwmRec> recs;
    DevBuf<unsigned char> h_in;                   // push_host(): the host window's device copy
    unsigned long long w0 = 0;                    // samples of the stream so far
    PwmPlan last{};                               // the most recent push's
    bool flushed = false;
    bool fetched = true;                          // `frames` / `bits` hold the most recent push's
    std::vector<rr_pwm_frame> frames;
    std::vector<unsigned char> bits;
    PwmDecoder(const PwmCfg& cfg, size_t es);
    void push_dev(const void* d_samples, size_t n, hipStream_t s);
    void push_host(const void* samples, size_t n);
    void flush(hipStream_t s);
    const std::vector<rr_pwm_frame>& fetch_frames();          // waits for the most recent push
    const std::vector<unsigned char>& fetch_bits();
private:
    void run(const void* d_samples, size_t n, bool eof, hipStream_t s);
};

// SymbolSync (symbol_sync.rs:46-217) x nstreams over windows of nstreams f32 streams (kernels_sync.hip): no stream protocol
// (work_dev is an error).  Each stream's state between pushes (SyncState) stays on the device; the host keeps only the geometry of
// the most recent push and clamps the counts it reads back to it (symsync_host.hpp).
struct SymbolSync : BatchBlock {
    SyncParams prm{};
    size_t nstreams;
    int spw;                                      // streams per wave of the clock kernel: 1 or 64
    int prof_launch;                              // rr_build_opts.sync_prof_launch: 1 .. 3 = profiling brackets that launch alone
    Carried<SyncState> st;                        // in(): what the streams so far left behind
    DevBuf<unsigned long long> words, count;      // the signs of the most recent push; symbols of each stream in it
    DevBuf<unsigned> idx;                         // the window-relative index of every emission, n slots per stream
    DevBuf<float> h_in, h_syms, h_clk;            // push_host(): the host buffers' device copies
    size_t last_n = 0;                            // the most recent push's window
    bool fetched = true;                          // `counts` holds the most recent push's
    std::vector<size_t> counts;
    SymbolSync(float sps, float max_deviation, const float* taps, size_t ntaps, size_t nstreams);
    void push_dev(const float* d_in, size_t in_stride, size_t n, float* d_syms, float* d_clock, size_t out_stride, hipStream_t s);
    void push_host(const float* in, size_t in_stride, size_t n, float* syms, float* clock, size_t out_stride, size_t* produced);
    const std::vector<size_t>& fetch_counts();                // waits for the most recent push
    SyncState fetch_state(size_t stream);                     // ... and downloads one stream's state
};

// BinarySlicer -> [XorConst(1)] -> [NrziDecode] -> [Descrambler] -> HdlcDeframer x nstreams over ragged windows of nstreams f32
// symbol streams (kernels_hdlcrx.hip): no stream protocol (work_dev is an error).  HdlcCore with the bit chain in front: the handle's
// own are each stream's chain state between pushes (RX_ST_*, with its position), the symbol source and the rr_hdlc_stream_frame records.
struct HdlcReceiver : BatchBlock {
    HdlcCore core;
    BitsCfg cfg{};                                // invert, nrzi, dmask
    Carried<unsigned long long> bst;              // in(): RX_ST_N words per stream
    DevBuf<HdlcRxRec> recs;
    DevBuf<float> h_syms;                         // push_host(): the host buffers' device copies
    DevBuf<unsigned long long> h_counts;
    bool fetched = true;                          // `frames` holds the most recent push's
    std::vector<rr_hdlc_stream_frame> frames;     // ... ascending by (stream, pos)
    HdlcReceiver(size_t nstreams, int bit_flags, unsigned long long mask, unsigned long long seed, unsigned len, size_t min_size,
                 size_t max_size, int hdlc_flags);
    void push_dev(const float* d_syms, size_t stride, size_t n_cap, const unsigned long long* d_counts, hipStream_t s);
    void push_host(const float* syms, size_t stride, size_t n_cap, const size_t* counts);
    const std::vector<rr_hdlc_stream_frame>& fetch_frames();  // waits for the most recent push
    const std::vector<unsigned char>& fetch_bytes();
    std::vector<unsigned long long> fetch_stats();            // 3 per stream
    std::vector<unsigned long long> fetch_consumed();         // 1 per stream
    std::vector<unsigned long long> positions(const unsigned long long* d_bst) const;    // RX_ST_POS of every stream, one download
};

// BinarySlicer -> [XorConst(1)] -> CorrelateAccessCodeTag(il2p SYNC_WORD) -> Il2pDeframer x nstreams over ragged windows of nstreams
// f32 symbol streams (kernels_il2p.hip, il2p_core.hpp): no stream protocol (work_dev is an error).  Each stream's state between
// pushes (IL2P_ST_*: position, bits seen, how far the open header blocks, the last IL2P_CARRY bits) stays on the device as a pair;
// the host keeps only the geometry of the most recent push.
struct Il2pReceiver : BatchBlock {
    size_t nstreams;
    int invert;
    unsigned allowed;                             // allowed_diffs, clamped to 24
    Carried<unsigned long long> st;               // in(): IL2P_ST_N words per stream
    DevBuf<unsigned long long> bits, mw, count, stats;   // stats: headers, syncs per stream since creation
    DevBuf<unsigned char> maps, entry;
    DevBuf<Il2pRec> recs;
    DevBuf<float> h_syms;                         // push_host(): the host buffers' device copies
    DevBuf<unsigned long long> h_counts;
    size_t last_n = 0;                            // n_cap of the most recent push
    bool fetched = true;                          // `headers` holds the most recent push's
    std::vector<rr_il2p_header> headers;          // ... ascending by (stream, pos)
    Il2pReceiver(size_t nstreams, int bit_flags, size_t allowed_diffs);
    void push_dev(const float* d_syms, size_t stride, size_t n_cap, const unsigned long long* d_counts, hipStream_t s);
    void push_host(const float* syms, size_t stride, size_t n_cap, const size_t* counts);
    const std::vector<rr_il2p_header>& fetch_headers();       // waits for the most recent push
    std::vector<unsigned long long> fetch_stats();            // 2 per stream
    std::vector<unsigned long long> fetch_consumed();         // 1 per stream
    std::vector<unsigned long long> positions(const unsigned long long* d_st) const;     // IL2P_ST_POS of every stream, one download
};

// Hilbert -> QuadratureDemod -> FftFilterFloat -> AddConst x nstreams over windows of nstreams f32 streams (kernels_afsk.hip,
// afsk_core.hpp): no stream protocol (work_dev is an error).  Each stream's latest L + H samples stay on the device between pushes;
// the host keeps only how many samples the streams have taken, which is all a push's counts depend on.
struct AfskDemod : BatchBlock {
    size_t nstreams;
    AfskGeom g{};
    float gain, offset;
    DevBuf<float> d_taps, d_hr;
    Carried<float> carry;                         // in(): nstreams x C, the streams' latest samples (zeros before their start)
    unsigned long long total = 0;                 // samples every stream has taken
    DevBuf<float> h_in, h_out;                    // push_host(): the host buffers' device copies
    AfskDemod(size_t nstreams, size_t hilbert_ntaps, int window, float window_parm, float gain, const float* taps, size_t ntaps,
              float offset);
    size_t push_dev(const float* d_in, size_t in_stride, size_t n, float* d_out, size_t out_stride, hipStream_t s);   // -> produced
    size_t push_host(const float* in, size_t in_stride, size_t n, float* out, size_t out_stride);
};

// norm -> FftFilterFloat -> RationalResampler -> MultiplyConst x nstreams over windows of nstreams Complex streams (kernels_am.hip,
// am_core.hpp): no stream protocol (work_dev is an error).  Each stream's latest L - 1 magnitudes stay on the device between
// pushes; the host keeps only where the resampler stands (e) and how many samples the streams have taken, which is all a push's
// counts depend on.
struct AmDemod : BatchBlock {
    size_t nstreams;
    AmGeom g{};
    float scale;
    DevBuf<float> d_taps;
    Carried<float> carry;                         // in(): nstreams x (L - 1), the streams' latest magnitudes (zeros before their start)
    long e = 0;                                   // output k of the next push sits over its sample (e + k D) / I
    unsigned long long total = 0;                 // samples every stream has taken
    DevBuf<float> h_out;                          // push_host(): the host buffers' device copies
    DevBuf<cf> h_in;
    AmDemod(size_t nstreams, const float* taps, size_t ntaps, size_t interp, size_t deci, float scale);
    size_t push_dev(const cf* d_in, size_t in_stride, size_t n, float* d_out, size_t out_stride, hipStream_t s);   // -> produced
    size_t push_host(const cf* in, size_t in_stride, size_t n, float* out, size_t out_stride);
};

// The modulators of the two packet transmitters over pushes of u8 line bits (kernels_tx.hip, fsk_core.hpp): no stream protocol
// (work_dev is an error).
//   AFSK    RationalResampler -> Map(bit > 0 ? hi : lo) -> Vco(k1) -> .re -> MultiplyConst(gain) -> RationalResampler -> Vco(k2)
//           (examples/bell202.rs:166-183)
//   DIRECT  RationalResampler -> Map -> Vco(k1) -> MultiplyConst(gain) -> RationalResampler (examples/g3ruh.rs:256-272)
// The two phases stay on the device between pushes; the host keeps where the two resamplers stand (FskPos), which is all a push's
// counts depend on.
struct FskTx : BatchBlock {
    int mode;
    FskRatio r1, r2;
    float lo, hi, gain;
    double k1, k2;
    FskPos pos;
    Carried<double> phase;                        // in(): phase 1, phase 2 behind the previous push's last sample (0 at start)
    DevBuf<unsigned> tilecnt;
    DevBuf<double> tiles2, pre2;
    DevBuf<float> audio;                          // a[] of a push that was given no d_audio
    DevBuf<cf> val;
    DevBuf<unsigned char> h_bits;                 // push_host(): the host buffers' device copies
    DevBuf<cf> h_out;
    DevBuf<float> h_audio;
    FskTx(int mode, size_t interp1, size_t deci1, float lo, float hi, double k1, float gain, size_t interp2, size_t deci2, double k2);
    FskPush count(size_t n_bits) const;           // the next push of n_bits; throws what that push would refuse for its length
    FskPush push_dev(const unsigned char* d_bits, size_t n_bits, cf* d_out, size_t out_cap, float* d_audio, size_t audio_cap,
                     hipStream_t s);
    FskPush push_host(const unsigned char* bits, size_t n_bits, cf* out, size_t out_cap, float* audio, size_t audio_cap);
};

// FskTx x nstreams of one parameter set over ragged pushes of u8 line bits, the counts read on the device (kernels_tx.hip,
// DESIGN.md 4.21): no stream protocol (work_dev is an error).  Every stream's FskPos and both its phases stay on the device; the
// host keeps the geometry of the most recent push and the sum of all n_cap, an upper bound of every stream's bit position.
struct FskTxMulti : BatchBlock {
    size_t nstreams;
    int mode;
    FskRatio r1, r2;
    float lo, hi, gain;
    double k1, k2;
    Carried<FskStream> st;                        // in(): what the streams so far left behind, one per stream
    DevBuf<FskPush> plan;                         // the most recent push of every stream, as the device planned it
    DevBuf<unsigned long long> made;              // [2][nstreams]: audio samples, then outputs, of every stream in it
    DevBuf<unsigned> tilecnt;
    DevBuf<double> tiles2, pre2;
    DevBuf<float> audio;                          // a[] of a push that was given no d_audio
    DevBuf<cf> val;
    DevBuf<unsigned char> h_bits;                 // push_host(): the host buffers' device copies
    DevBuf<unsigned long long> h_counts;
    DevBuf<cf> h_out;
    DevBuf<float> h_audio;
    unsigned long long bits_bound = 0;            // the sum of the n_cap of all pushes
    size_t last_audio_cap = 0, last_out_cap = 0;  // the bound of the most recent push
    bool fetched = true;                          // `counts` holds the most recent push's
    std::vector<unsigned long long> counts;       // [2][nstreams], checked against the bound
    FskTxMulti(size_t nstreams, int mode, size_t interp1, size_t deci1, float lo, float hi, double k1, float gain, size_t interp2,
               size_t deci2, double k2);
    void push_dev(const unsigned char* d_bits, size_t bits_stride, size_t n_cap, const unsigned long long* d_counts, cf* d_out,
                  size_t out_stride, float* d_audio, size_t audio_stride, hipStream_t s);
    void push_host(const unsigned char* bits, size_t bits_stride, size_t n_cap, const size_t* counts, cf* out, size_t out_stride,
                   float* audio, size_t audio_stride, size_t* n_out, size_t* n_audio);
    const std::vector<unsigned long long>& fetch_counts();    // waits for the most recent push
    std::vector<FskStream> fetch_state();                     // ... and downloads every stream's state
};

}  // namespace rr
