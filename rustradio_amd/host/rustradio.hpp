// rustradio.hpp — C++17 host-side mirror of rustradio's operator API for the hot path,
// layered on the C ABI (include/rustradio_amd.h).  The reference is Rust; this image has no
// Rust toolchain, so the host side above the C ABI is C++ with the same names, argument
// meaning and error behaviour as the reference:
//
//   Block / BlockRet / BlockName / BlockEOF      src/block.rs:12-126
//   ReadStream / WriteStream / Tag / new_stream  src/stream.rs:48-93, 105, 187-339
//   VectorSource / VectorSink / NullSink / Graph  src/vector_source.rs, src/vector_sink.rs,
//                                                 src/null_sink.rs, src/graph.rs:99-173
//   FirFilter (+builder .deci() .translate()), Fir::filter_n   src/fir.rs:150-198, 303-551
//   FftFilter / FftFilterFloat                    src/fft_filter.rs:210-491
//   RationalResampler (+builder)                  src/rational_resampler.rs:19-213
//   QuadratureDemod                               src/quadrature_demod.rs:32-114
//   Hilbert                                       src/hilbert.rs:22-129
//   fir::low_pass / low_pass_complex / hilbert, window::WindowType   src/fir.rs:594-680, src/window.rs
//
// A block's work() does exactly what the Rust shim in INTEGRATION.md does: take the stream
// windows, hand plain pointers to rr_block_work(), then consume()/produce() what the GPU
// block reported, re-basing tags the way the reference block does.  No sample arithmetic
// happens in this file.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <type_traits>
#include <variant>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include "../../include/rustradio_amd.h"

namespace rustradio {

using Float = float;                    // src/lib.rs:268
using Complex = std::complex<float>;    // src/lib.rs:271 (interleaved re, im)

struct Error : std::runtime_error {     // src/lib.rs:276-311
    using std::runtime_error::runtime_error;
    static Error msg(const std::string& m) { return Error(m); }
};

constexpr size_t DEFAULT_STREAM_SIZE = 4'096'000;   // bytes, src/stream.rs:105

// ---- tags (src/stream.rs:48-93) ----------------------------------------------------------------
using TagValue = std::variant<bool, uint64_t, float, std::string>;
struct Tag {
    size_t pos_;
    std::string key_;
    TagValue val_;
    Tag(size_t p, std::string k, TagValue v) : pos_(p), key_(std::move(k)), val_(std::move(v)) {}
    size_t pos() const { return pos_; }
    void set_pos(size_t p) { pos_ = p; }
    const std::string& key() const { return key_; }
    const TagValue& val() const { return val_; }
    bool operator==(const Tag& o) const { return pos_ == o.pos_ && key_ == o.key_ && val_ == o.val_; }
};

namespace detail {
inline uint64_t& activity() { static thread_local uint64_t a = 0; return a; }   // samples moved (Graph idle detection)
}

// ---- streams --------------------------------------------------------------------------------------
// The reference hands out contiguous windows of a double-mapped ring shared by a ReadStream and a
// WriteStream that may live on different threads (src/nowasm/circular_buffer.rs:98-128, 572-615).
// This harness does the same: one memfd mapped twice back to back, read_buf() = ALL readable samples,
// write_buf() = ALL free space, fixed capacity; counters and tags under one lock, windows stable while
// the other end works, a condition variable behind StreamWait::wait (src/stream.rs:114-138).
struct StreamWait {
    virtual ~StreamWait() = default;
    virtual size_t id() const = 0;
    // true = `need` will never be satisfied: go ahead and EOF (stream.rs:121-126)
    virtual bool wait(size_t need) const = 0;
    virtual bool closed() const = 0;
};

// Where new_stream() places rings.  Memory::Device = an HBM-resident ring (rr_dstream): GPU
// blocks chained through such streams run rr_block_work_dev on the windows — no PCIe hop and no
// host/device synchronisation per work(); only sources (fill_from_slice) and sinks (copy_to) cross
// the bus.  Tags stay a host-side side-band in both cases.  Set once before building a graph.
enum class Memory { Host, Device };
inline Memory& default_memory() { static thread_local Memory m = Memory::Host; return m; }

namespace detail {
// How long one StreamWait::wait sleeps at most before it reports back (the reference's condvar wait has no
// timeout because every produce / consume / drop notifies; so does this one — the timeout only bounds a lost race).
constexpr unsigned WAIT_SLICE_MS = 100;
// One physical range mapped at two consecutive virtual ranges (circular_buffer.rs:98-128).
struct DoubleMap {
    unsigned char* base = nullptr;
    size_t phys = 0;
    explicit DoubleMap(size_t bytes) {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        phys = std::max(page, (bytes + page - 1) / page * page);
        const int fd = memfd_create("rustradio_ring", 0);
        if (fd < 0 || ftruncate(fd, (off_t)phys) != 0) { if (fd >= 0) close(fd); throw Error("stream ring: memfd_create failed"); }
        void* va = mmap(nullptr, 2 * phys, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        bool ok = va != MAP_FAILED;
        ok = ok && mmap(va, phys, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, fd, 0) != MAP_FAILED;
        ok = ok && mmap((unsigned char*)va + phys, phys, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, fd, 0) != MAP_FAILED;
        close(fd);
        if (!ok) { if (va != MAP_FAILED) munmap(va, 2 * phys); throw Error("stream ring: mmap failed"); }
        base = static_cast<unsigned char*>(va);
    }
    ~DoubleMap() { if (base) munmap(base, 2 * phys); }
    DoubleMap(const DoubleMap&) = delete;
};
}  // namespace detail

template <class T> struct StreamState {
    std::unique_ptr<detail::DoubleMap> ring;   // host ring: bytes [rb, rb + used * sizeof(T)) readable
    size_t rb = 0, used_ = 0;
    rr_dstream* ds = nullptr;     // device ring (then `ring` is unused; its counters live in the library, under its own lock)
    size_t cap;
    std::vector<Tag> tags;        // positions relative to the read window
    bool writer_alive = true, reader_alive = true;
    size_t id_;
    mutable std::mutex m;         // rb, used_, tags, the two flags
    mutable std::condition_variable cv;
    // the two ends as StreamWait objects: BlockRet::WaitForStream carries one of them (block.rs:61)
    struct Side : StreamWait {
        const StreamState* st; bool reader;
        Side(const StreamState* s, bool r) : st(s), reader(r) {}
        size_t id() const override { return st->id_; }
        bool closed() const override { return st->closed(); }
        bool wait(size_t need) const override { return st->wait(reader, need); }
    } rside{this, true}, wside{this, false};
    explicit StreamState(size_t bytes, Memory m_ = default_memory()) : cap(bytes / sizeof(T)) {
        static std::atomic<size_t> next_id{1};
        id_ = next_id++;
        if (cap == 0) throw Error("stream: capacity smaller than one sample");
        if (m_ == Memory::Device) {
            ds = rr_dstream_create(sizeof(T), bytes);
            if (!ds) throw Error(rr_last_error());
        } else {
            ring = std::make_unique<detail::DoubleMap>(cap * sizeof(T));
            // page-lock the whole double mapping once: GPU blocks then read and write the windows of this
            // ring in place over PCIe (zero copy).  Without a GPU the call fails and the ring is an ordinary host ring.
            registered = rr_host_register(ring->base, 2 * ring->phys) == 0;
        }
    }
    ~StreamState() {
        if (ds) rr_dstream_destroy(ds);
        if (registered) rr_host_unregister(ring->base);
    }
    bool registered = false;
    StreamState(const StreamState&) = delete;
    bool device() const { return ds != nullptr; }
    size_t used() const {
        if (ds) return rr_dstream_read_buf(ds, nullptr);
        std::lock_guard<std::mutex> g(m);
        return used_;
    }
    size_t free() const { return cap - used(); }
    bool closed() const {                                    // src/stream.rs:148-150,166-168: the other end is gone
        std::lock_guard<std::mutex> g(m);
        return !writer_alive || !reader_alive;
    }
    void drop_end(bool reader) {
        { std::lock_guard<std::mutex> g(m); (reader ? reader_alive : writer_alive) = false; }
        if (ds) rr_dstream_close(ds, reader ? RR_SIDE_READER : RR_SIDE_WRITER);
        cv.notify_all();
    }
    // wait_for_read / wait_for_write (stream.rs:222-224,311-313): what is there < need AND the other end dropped
    bool wait(bool reader, size_t need) const {
        if (ds) {
            int never = 0;
            rr_dstream_wait(ds, reader ? RR_SIDE_READER : RR_SIDE_WRITER, need, detail::WAIT_SLICE_MS, &never);
            return never != 0;
        }
        std::unique_lock<std::mutex> g(m);
        auto have = [&] { return reader ? used_ : cap - used_; };
        auto other_gone = [&] { return reader ? !writer_alive : !reader_alive; };
        cv.wait_for(g, std::chrono::milliseconds(detail::WAIT_SLICE_MS), [&] { return have() >= need || other_gone(); });
        return have() < need && other_gone();
    }
};

template <class T> class BufferReader {   // circular_buffer.rs:233-251
    std::shared_ptr<StreamState<T>> s_;
    const T* ptr_ = nullptr;      // the window as it was when read_buf() was called (host or DEVICE pointer)
    size_t len_ = 0;
public:
    explicit BufferReader(std::shared_ptr<StreamState<T>> s) : s_(std::move(s)) {
        if (s_->ds) {
            const void* p = nullptr;
            len_ = rr_dstream_read_buf(s_->ds, &p);
            ptr_ = static_cast<const T*>(p);
        } else {
            std::lock_guard<std::mutex> g(s_->m);
            ptr_ = reinterpret_cast<const T*>(s_->ring->base + s_->rb);
            len_ = s_->used_;
        }
    }
    bool device() const { return s_->device(); }
    const T* slice() const { return ptr_; }
    size_t len() const { return len_; }
    bool is_empty() const { return len() == 0; }
    const T* begin() const { host_only(); return slice(); }
    const T* end() const { host_only(); return slice() + len(); }
    // first n samples of the window into host memory (any placement)
    rr_dstream* dstream() const { return s_->ds; }
    void copy_to(T* host, size_t n) const {
        if (n > len()) throw Error("copy_to: n > readable");
        if (!s_->ds) { if (n) std::memcpy(host, slice(), n * sizeof(T)); return; }
        if (rr_dstream_copy_out(s_->ds, 0, host, n, nullptr) != 0) throw Error(rr_last_error());
    }
    void consume(size_t n) {               // circular_buffer.rs:472-513
        if (n > len_) throw Error("consume: n > used");
        detail::activity() += n;
        {
            std::lock_guard<std::mutex> g(s_->m);
            std::vector<Tag> keep;
            for (auto& t : s_->tags)
                if (t.pos() >= n) keep.emplace_back(t.pos() - n, t.key(), t.val());
            s_->tags.swap(keep);
            if (!s_->ds) {
                s_->rb = (s_->rb + n * sizeof(T)) % s_->ring->phys;
                s_->used_ -= n;
            } else if (rr_dstream_consume(s_->ds, n) != 0) {   // under m, like produce: tags and the ring's counters move together
                throw Error(rr_last_error());
            }
        }
        ptr_ += n; len_ -= n;
        if (n) s_->cv.notify_all();
    }
private:
    void host_only() const { if (s_->ds) throw Error("host iteration over a device-resident stream: use copy_to()"); }
};

template <class T> class BufferWriter {   // circular_buffer.rs:284-310
    std::shared_ptr<StreamState<T>> s_;
    T* ptr_ = nullptr;            // the write window as it was when write_buf() was called (host or DEVICE pointer)
    size_t len_ = 0;
public:
    explicit BufferWriter(std::shared_ptr<StreamState<T>> s) : s_(std::move(s)) {
        if (s_->ds) {
            void* p = nullptr;
            len_ = rr_dstream_write_buf(s_->ds, &p, nullptr);
            ptr_ = static_cast<T*>(p);
            return;
        }
        std::lock_guard<std::mutex> g(s_->m);
        ptr_ = reinterpret_cast<T*>(s_->ring->base + (s_->rb + s_->used_ * sizeof(T)) % s_->ring->phys);
        len_ = s_->cap - s_->used_;
    }
    BufferWriter(BufferWriter&& o) noexcept : s_(std::move(o.s_)), ptr_(o.ptr_), len_(o.len_) { o.s_.reset(); }
    BufferWriter(const BufferWriter&) = delete;
    bool device() const { return s_->device(); }
    T* slice() { return ptr_; }                                         // host or DEVICE pointer
    size_t len() const { return len_; }
    bool is_empty() const { return len() == 0; }
    // n samples of a DEVICE-resident read window into this DEVICE-resident write window: no host hop (rr_dstream_copy)
    void fill_from_device(const BufferReader<T>& src, size_t n) {
        if (n > len()) throw Error("fill_from_device: n > free");
        if (!s_->ds || !src.dstream()) throw Error("fill_from_device: both streams must be device-resident");
        if (rr_dstream_copy(s_->ds, 0, src.dstream(), 0, n, nullptr) != 0) throw Error(rr_last_error());
    }
    void fill_from_slice(const T* src, size_t n) {                      // src = host memory
        if (n > len()) throw Error("fill_from_slice: n > free");
        if (!s_->ds) { if (n) std::memcpy(slice(), src, n * sizeof(T)); return; }
        if (rr_dstream_copy_in(s_->ds, 0, src, n, nullptr) != 0) throw Error(rr_last_error());
    }
    void produce(size_t n, const std::vector<Tag>& tags) {   // circular_buffer.rs:518-557
        if (n > len()) throw Error("produce: n > free");
        if (n == 0) return;                                  // tags dropped (:528-533)
        detail::activity() += n;
        {
            // tag positions are relative to the READ window as it is now (the reader may have consumed since write_buf())
            std::lock_guard<std::mutex> g(s_->m);
            const size_t base = s_->ds ? rr_dstream_read_buf(s_->ds, nullptr) : s_->used_;
            for (auto& t : tags) s_->tags.emplace_back(t.pos() + base, t.key(), t.val());
            if (!s_->ds) s_->used_ += n;
            else if (rr_dstream_produce(s_->ds, n) != 0) throw Error(rr_last_error());
        }
        ptr_ += n; len_ -= n;
        s_->cv.notify_all();
    }
};

template <class T> class ReadStream {      // src/stream.rs:187-246
    std::shared_ptr<StreamState<T>> s_;
public:
    ReadStream() = default;
    explicit ReadStream(std::shared_ptr<StreamState<T>> s) : s_(std::move(s)) {}
    ~ReadStream() { if (s_) s_->drop_end(true); }
    ReadStream(ReadStream&&) = default;
    ReadStream& operator=(ReadStream&&) = default;
    ReadStream(const ReadStream&) = delete;
    static ReadStream from_slice(const T* d, size_t n) {    // src/stream.rs:187-195 (test helper)
        auto st = std::make_shared<StreamState<T>>(DEFAULT_STREAM_SIZE, Memory::Host);
        if (n > st->cap) throw Error("from_slice: more samples than the ring holds");
        if (n) std::memcpy(st->ring->base, d, n * sizeof(T));
        st->used_ = n;
        st->writer_alive = false;
        return ReadStream(st);
    }
    std::pair<BufferReader<T>, std::vector<Tag>> read_buf() const {   // :208-217
        BufferReader<T> r(s_);
        std::lock_guard<std::mutex> g(s_->m);
        std::vector<Tag> t;
        for (auto& x : s_->tags) if (x.pos() < r.len()) t.push_back(x);
        return {std::move(r), std::move(t)};
    }
    bool eof() const {                                                 // :237-246: writer gone and nothing left
        { std::lock_guard<std::mutex> g(s_->m); if (s_->writer_alive) return false; }
        return s_->used() == 0;
    }
    const StreamWait& wait_handle() const { return s_->rside; }
    size_t id() const { return s_->id_; }
};

template <class T> class WriteStream {     // src/stream.rs:288-310
    std::shared_ptr<StreamState<T>> s_;
public:
    WriteStream() = default;
    explicit WriteStream(std::shared_ptr<StreamState<T>> s) : s_(std::move(s)) {}
    ~WriteStream() { if (s_) s_->drop_end(false); }
    WriteStream(WriteStream&&) = default;
    WriteStream& operator=(WriteStream&&) = default;
    WriteStream(const WriteStream&) = delete;
    BufferWriter<T> write_buf() const { return BufferWriter<T>(s_); }  // :301-310
    size_t free() const { return s_->free(); }
    const StreamWait& wait_handle() const { return s_->wside; }
    size_t id() const { return s_->id_; }
};

// Ring size used by new_stream() when none is given.  The reference's 4,096,000 bytes suit CPU caches; rings
// in HBM want hundreds of MB so that one work() is milliseconds, not microseconds, of kernel.
inline size_t& default_stream_size() { static thread_local size_t b = DEFAULT_STREAM_SIZE; return b; }

template <class T> std::pair<WriteStream<T>, ReadStream<T>> new_stream(size_t bytes = default_stream_size(),
                                                                       Memory m = default_memory()) {  // :336-339
    auto st = std::make_shared<StreamState<T>>(bytes, m);
    return {WriteStream<T>(st), ReadStream<T>(st)};
}

// ---- Block (src/block.rs) -----------------------------------------------------------------------------
struct BlockRet {
    enum Kind { Again, Pending, WaitForStream, EOF_ } kind;
    const StreamWait* stream = nullptr;
    size_t need = 0;
    static BlockRet again() { return {Again, nullptr, 0}; }
    static BlockRet eof() { return {EOF_, nullptr, 0}; }
    static BlockRet wait(const StreamWait& s, size_t n) { return {WaitForStream, &s, n}; }
};

struct Block {
    virtual ~Block() = default;
    virtual const char* block_name() const = 0;   // BlockName, :91-97
    virtual bool eof() = 0;                       // BlockEOF, :103-110
    virtual BlockRet work() = 0;                  // Block::work, :115-126 (throws Error on failure)
};

// ---- window / tap designers (src/window.rs, src/fir.rs:594-680) -----------------------------------------
namespace window {
struct WindowType {
    int kind; float parm;
    static WindowType Hamming() { return {RR_WIN_HAMMING, 0}; }
    static WindowType Blackman() { return {RR_WIN_BLACKMAN, 0}; }
    static WindowType BlackmanHarris() { return {RR_WIN_BLACKMAN_HARRIS, 0}; }
    static WindowType HammingParm(float a0) { return {RR_WIN_HAMMING_PARM, a0}; }
    float max_attenuation() const { return rr_max_attenuation(kind); }
    std::vector<Float> make_window(size_t ntaps) const {
        std::vector<Float> w(ntaps);
        if (rr_make_window(kind, parm, ntaps, w.data()) != 0) throw Error(rr_last_error());
        return w;
    }
};
}  // namespace window

namespace fir {
inline std::vector<Float> low_pass(Float samp_rate, Float cutoff, Float twidth, const window::WindowType& w) {
    const size_t n = rr_low_pass(samp_rate, cutoff, twidth, w.kind, w.parm, nullptr, 0);
    if (n == 0) throw Error(rr_last_error());       // the reference asserts (fir.rs:623-625)
    std::vector<Float> t(n);
    rr_low_pass(samp_rate, cutoff, twidth, w.kind, w.parm, t.data(), n);
    return t;
}
inline std::vector<Complex> low_pass_complex(Float samp_rate, Float cutoff, Float twidth, const window::WindowType& w) {
    auto t = low_pass(samp_rate, cutoff, twidth, w);
    return std::vector<Complex>(t.begin(), t.end());   // Complex::new(t, 0.0), fir.rs:602
}
inline std::vector<Float> hilbert(const std::vector<Float>& window) {
    std::vector<Float> t(window.size());
    if (rr_hilbert_taps(window.data(), window.size(), t.data()) != 0) throw Error(rr_last_error());
    return t;
}
}  // namespace fir

// ---- GPU block plumbing -----------------------------------------------------------------------------------
namespace detail {
struct Handle {
    rr_block* h;
    explicit Handle(rr_block* p) : h(p) { if (!h) throw Error(rr_last_error()); }
    ~Handle() { rr_block_destroy(h); }
    Handle(const Handle&) = delete;
};
struct WorkOut { int st; size_t consumed, produced, need; };
inline WorkOut work(rr_block* h, const void* in, size_t in_len, void* out, size_t out_cap) {
    WorkOut w{};
    w.st = rr_block_work(h, in, in_len, out, out_cap, &w.consumed, &w.produced, &w.need);
    if (w.st == RR_ERR) throw Error(rr_last_error());
    return w;
}
// Block::work() over a read and a write window of the same placement: host windows go through
// rr_block_work (PCIe round trip inside), device windows through rr_block_work_dev on the default stream.
template <class I, class O> inline WorkOut work(rr_block* h, const BufferReader<I>& in, BufferWriter<O>& out) {
    if (in.device() != out.device())
        throw Error("a GPU block needs both streams in the same memory: put a MemCopy block in between");
    if (!in.device()) return work(h, in.slice(), in.len(), out.slice(), out.len());
    WorkOut w{};
    w.st = rr_block_work_dev(h, in.slice(), in.len(), out.slice(), out.len(), &w.consumed, &w.produced, &w.need, nullptr);
    if (w.st == RR_ERR) throw Error(rr_last_error());
    return w;
}
static_assert(sizeof(Complex) == sizeof(rr_c32), "Complex<f32> must be interleaved re, im");

// Tags through a block that is known only by its handle (Fused, GpuResident): the reference rule of the block(s) behind the
// handle, as rr_block_tag_rule states it in whole-stream positions.  step() takes the tags of the read window (positions
// relative to it; only those on consumed samples travel, the rest stay in the stream) and returns the tags of the
// `produced` outputs of this call (positions relative to them).  A tag whose output sample does not exist yet waits here,
// as it does in FftFilter's `self.tags` (fft_filter.rs:309-313).
class TagForwarder {
    int rule_ = RR_TAGS_DROP;
    size_t param_ = 1;
    std::vector<std::pair<uint64_t, Tag>> pending_;   // (output position counted from the start of the stream, tag)
    uint64_t in_abs_ = 0, out_abs_ = 0;
public:
    explicit TagForwarder(const rr_block* h) {
        size_t p = 1;
        rule_ = rr_block_tag_rule(h, &p);
        if (rule_ == RR_ERR) throw Error(rr_last_error());
        param_ = p || rule_ == RR_TAGS_SHIFT ? p : 1;
    }
    bool drops() const { return rule_ == RR_TAGS_DROP; }
    std::vector<Tag> step(const std::vector<Tag>& tags, size_t consumed, size_t produced) {
        std::vector<Tag> emit;
        if (rule_ == RR_TAGS_FORWARD) {
            for (auto& t : tags)
                if (t.pos() < consumed) pending_.emplace_back((in_abs_ + t.pos()) / param_, t);
            std::vector<std::pair<uint64_t, Tag>> keep;
            for (auto& pt : pending_) {
                if (pt.first < out_abs_ + produced) emit.emplace_back((size_t)(pt.first - out_abs_), pt.second.key(), pt.second.val());
                else keep.push_back(std::move(pt));
            }
            pending_.swap(keep);
        } else if (rule_ == RR_TAGS_SHIFT) {              // delay.rs:104-108: *param outputs precede the first copied sample
            for (auto& t : tags)
                if (t.pos() < consumed) pending_.emplace_back(in_abs_ + t.pos() + param_, t);
            std::vector<std::pair<uint64_t, Tag>> keep;
            for (auto& pt : pending_) {
                if (pt.first < out_abs_ + produced) emit.emplace_back((size_t)(pt.first - out_abs_), pt.second.key(), pt.second.val());
                else keep.push_back(std::move(pt));
            }
            pending_.swap(keep);
        } else if (rule_ == RR_TAGS_FRAMES) {             // fft_stream.rs:98-111 (produced is a whole number of frames)
            for (size_t pos = 0; pos + param_ <= produced; pos += param_) {
                emit.emplace_back(pos, "FftStream::size", (uint64_t)param_);
                emit.emplace_back(pos, "FftStream::frame", true);
                emit.emplace_back(pos + param_ - 1, "FftStream::frame", false);
            }
        }
        in_abs_ += consumed;
        out_abs_ += produced;
        return emit;
    }
};
}  // namespace detail

// ---- FirFilter (src/fir.rs) ---------------------------------------------------------------------------------
template <class T> class FirFilter;

template <class T> class FirFilterBuilder {      // fir.rs:303-340, 476-486
    std::vector<T> taps_;
    size_t deci_ = 1;
    bool translate_ = false;
    Float samp_rate_ = 0, freq_ = 0;
    friend class FirFilter<T>;
public:
    explicit FirFilterBuilder(std::vector<T> taps) : taps_(std::move(taps)) {}
    FirFilterBuilder& deci(size_t d) { if (d == 0) throw Error("FirFilter: deci 0"); deci_ = d; return *this; }
    FirFilterBuilder& translate(Float samp_rate, Float freq) {
        static_assert(std::is_same<T, Complex>::value, "FirFilter asked to translate on non-Complex");
        translate_ = true; samp_rate_ = samp_rate; freq_ = freq; return *this;
    }
    std::pair<std::unique_ptr<FirFilter<T>>, ReadStream<T>> build(ReadStream<T> src);
};

template <class T> class FirFilter : public Block {
    detail::Handle h_;
    size_t deci_;
    ReadStream<T> src_;
    WriteStream<T> dst_;
    static rr_block* make(const std::vector<T>& taps, size_t deci, bool tr, Float fs, Float f) {
        if constexpr (std::is_same<T, Complex>::value)
            return rr_fir_c32_create(reinterpret_cast<const rr_c32*>(taps.data()), taps.size(), deci, tr, fs, f);
        else
            return rr_fir_f32_create(taps.data(), taps.size(), deci);
    }
public:
    FirFilter(ReadStream<T> src, WriteStream<T> dst, const FirFilterBuilder<T>& b)
        : h_(make(b.taps_, b.deci_, b.translate_, b.samp_rate_, b.freq_)), deci_(b.deci_), src_(std::move(src)), dst_(std::move(dst)) {}
    static FirFilterBuilder<T> builder(std::vector<T> taps) { return FirFilterBuilder<T>(std::move(taps)); }
    static std::pair<std::unique_ptr<FirFilter<T>>, ReadStream<T>> new_(ReadStream<T> src, std::vector<T> taps) {
        return FirFilterBuilder<T>(std::move(taps)).build(std::move(src));
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {                    // fir.rs:492-550
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        if (w.st == RR_WAIT_SRC) { out.produce(0, {}); return BlockRet::wait(src_.wait_handle(), w.need); }
        if (w.st == RR_WAIT_DST) { out.produce(0, {}); return BlockRet::wait(dst_.wait_handle(), w.need); }
        std::vector<Tag> keep;                    // :536-545
        for (auto& t : tags)
            if (t.pos() < w.consumed) keep.emplace_back(t.pos() / deci_, t.key(), t.val());
        input.consume(w.consumed);
        out.produce(w.produced, keep);
        return BlockRet::again();
    }
};
template <class T>
std::pair<std::unique_ptr<FirFilter<T>>, ReadStream<T>> FirFilterBuilder<T>::build(ReadStream<T> src) {
    if (taps_.empty()) throw Error("FirFilter: empty taps");
    auto [w, r] = new_stream<T>();
    return {std::make_unique<FirFilter<T>>(std::move(src), std::move(w), *this), std::move(r)};
}

// Fir<T>::filter_n (fir.rs:181-189): `filter()` across an input range; runs the same HIP kernel.
template <class T> class Fir {
    std::vector<T> taps_;
public:
    explicit Fir(std::vector<T> taps) : taps_(std::move(taps)) { if (taps_.empty()) throw Error("Fir: empty taps"); }
    std::vector<T> filter_n(const std::vector<T>& input, size_t deci) const {
        if (deci == 0) throw Error("filter_n: deci 0");
        if (input.size() < taps_.size()) throw Error("filter_n: input shorter than taps");
        const size_t n_out = (input.size() - taps_.size()) / deci + 1;
        // pad so that the block's "consume whole groups of deci" rule (fir.rs:502) covers n_out outputs
        std::vector<T> in(input);
        in.resize((n_out - 1) * deci + taps_.size() + deci - 1, T{});
        detail::Handle h(FirFilterMaker(taps_, deci));
        std::vector<T> out(n_out);
        auto w = detail::work(h.h, in.data(), in.size(), out.data(), out.size());
        if (w.st != RR_AGAIN || w.produced != n_out) throw Error("filter_n: unexpected block state");
        return out;
    }
    // filter_n_inplace (fir.rs:191-197): out.size() outputs, out[i] = filter(&input[i * deci ..])
    void filter_n_inplace(const std::vector<T>& input, size_t deci, std::vector<T>& out) const {
        if (out.empty()) return;
        if (input.size() < (out.size() - 1) * deci + taps_.size()) throw Error("filter_n_inplace: input too short");
        std::vector<T> in(input.begin(), input.begin() + (std::ptrdiff_t)((out.size() - 1) * deci + taps_.size()));
        const auto r = filter_n(in, deci);
        std::copy(r.begin(), r.begin() + (std::ptrdiff_t)out.size(), out.begin());
    }
    // filter (fir.rs:166-177): one output from the first taps.size() samples
    T filter(const std::vector<T>& input) const { return filter_n(std::vector<T>(input.begin(), input.begin() + (std::ptrdiff_t)taps_.size()), 1)[0]; }
private:
    static rr_block* FirFilterMaker(const std::vector<T>& taps, size_t deci) {
        if constexpr (std::is_same<T, Complex>::value)
            return rr_fir_c32_create(reinterpret_cast<const rr_c32*>(taps.data()), taps.size(), deci, 0, 0, 0);
        else
            return rr_fir_f32_create(taps.data(), taps.size(), deci);
    }
};

// ---- FftFilter / FftFilterFloat (src/fft_filter.rs) ---------------------------------------------------------------
template <class T> class FftFilterBase : public Block {
protected:
    detail::Handle h_;
    ReadStream<T> src_;
    WriteStream<T> dst_;
    detail::TagForwarder fwd_;                        // tags of samples still inside `buf` wait here (:309-313)
public:
    FftFilterBase(rr_block* h, ReadStream<T> src, WriteStream<T> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)), fwd_(h_.h) {}
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {                    // fft_filter.rs:290-354 / 429-490
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        // a tag travels with its sample: output sample i is input sample i of the stream
        const std::vector<Tag> emit = fwd_.step(tags, w.consumed, w.produced);
        input.consume(w.consumed);
        out.produce(w.produced, emit);
        if (w.st == RR_WAIT_SRC) return BlockRet::wait(src_.wait_handle(), w.need);
        if (w.st == RR_WAIT_DST) return BlockRet::wait(dst_.wait_handle(), w.need);
        return BlockRet::again();
    }
};

class FftFilter : public FftFilterBase<Complex> {
public:
    using FftFilterBase<Complex>::FftFilterBase;
    static std::pair<std::unique_ptr<FftFilter>, ReadStream<Complex>> new_(ReadStream<Complex> src, const std::vector<Complex>& taps) {
        auto [w, r] = new_stream<Complex>();
        rr_block* h = rr_fftfilter_create(reinterpret_cast<const rr_c32*>(taps.data()), taps.size());
        return {std::make_unique<FftFilter>(h, std::move(src), std::move(w)), std::move(r)};
    }
};
class FftFilterFloat : public FftFilterBase<Float> {
public:
    using FftFilterBase<Float>::FftFilterBase;
    static std::pair<std::unique_ptr<FftFilterFloat>, ReadStream<Float>> new_(ReadStream<Float> src, const std::vector<Float>& taps) {
        auto [w, r] = new_stream<Float>();
        rr_block* h = rr_fftfilter_float_create(taps.data(), taps.size());
        return {std::make_unique<FftFilterFloat>(h, std::move(src), std::move(w)), std::move(r)};
    }
};

// ---- RationalResampler (src/rational_resampler.rs) ------------------------------------------------------------------
template <class T> class RationalResampler : public Block {
    detail::Handle h_;
    ReadStream<T> src_;
    WriteStream<T> dst_;
public:
    RationalResampler(rr_block* h, ReadStream<T> src, WriteStream<T> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)) {}
    // Err (here: throws Error) when interp or deci is 0 (:130-135)
    static std::pair<std::unique_ptr<RationalResampler<T>>, ReadStream<T>> new_(ReadStream<T> src, size_t interp, size_t deci) {
        auto [w, r] = new_stream<T>();
        rr_block* h = rr_resampler_create(interp, deci, sizeof(T));
        return {std::make_unique<RationalResampler<T>>(h, std::move(src), std::move(w)), std::move(r)};
    }
    struct Builder {                              // typestate builder (:19-92), flattened
        size_t interp_ = 0, deci_ = 0;
        Builder& interp(size_t i) { interp_ = i; return *this; }
        Builder& deci(size_t d) { deci_ = d; return *this; }
        auto build(ReadStream<T> src) { return RationalResampler<T>::new_(std::move(src), interp_, deci_); }
    };
    static Builder builder() { return Builder{}; }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }   // pending.is_none() && src.eof() (:209-213)
    BlockRet work() override {                    // :155-206 — tags are dropped (:156)
        auto [input, tags] = src_.read_buf();
        (void)tags;
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        input.consume(w.consumed);
        out.produce(w.produced, {});
        return w.st == RR_WAIT_DST ? BlockRet::wait(dst_.wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
};

// ---- QuadratureDemod (src/quadrature_demod.rs) -------------------------------------------------------------------------
class QuadratureDemod : public Block {
    detail::Handle h_;
    ReadStream<Complex> src_;
    WriteStream<Float> dst_;
public:
    QuadratureDemod(rr_block* h, ReadStream<Complex> src, WriteStream<Float> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)) {}
    // `exact_atan2 = true` is a --no-default-features build (f32::atan2); false = fast-math feature
    static std::pair<std::unique_ptr<QuadratureDemod>, ReadStream<Float>> new_(ReadStream<Complex> src, Float gain, bool exact_atan2 = true) {
        auto [w, r] = new_stream<Float>();
        rr_block* h = rr_quaddemod_create(gain, exact_atan2 ? RR_ATAN2_EXACT : RR_ATAN2_FAST);
        return {std::make_unique<QuadratureDemod>(h, std::move(src), std::move(w)), std::move(r)};
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {                    // :46-113 — tags dropped
        auto [input, tags] = src_.read_buf();
        (void)tags;
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        input.consume(w.consumed);
        out.produce(w.produced, {});
        return w.st == RR_WAIT_DST ? BlockRet::wait(dst_.wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
};

// ---- RtlSdrDecode (src/rtlsdr_decode.rs) ----------------------------------------------------------------------------------
class RtlSdrDecode : public Block {
    detail::Handle h_;
    ReadStream<uint8_t> src_;
    WriteStream<Complex> dst_;
public:
    RtlSdrDecode(rr_block* h, ReadStream<uint8_t> src, WriteStream<Complex> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)) {}
    static std::pair<std::unique_ptr<RtlSdrDecode>, ReadStream<Complex>> new_(ReadStream<uint8_t> src) {   // #[rustradio(new)], :9-16
        auto [w, r] = new_stream<Complex>();
        return {std::make_unique<RtlSdrDecode>(rr_rtlsdr_decode_create(), std::move(src), std::move(w)), std::move(r)};
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {                    // :18-47 — tags dropped (":21 TODO: handle tags")
        auto [input, tags] = src_.read_buf();
        (void)tags;
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        input.consume(w.consumed);
        out.produce(w.produced, {});
        return w.st == RR_WAIT_DST ? BlockRet::wait(dst_.wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
};

// ---- FftStream (src/fft_stream.rs) -------------------------------------------------------------------------------------------
inline constexpr const char* TAG_FRAME = "FftStream::frame";            // :18
inline constexpr const char* TAG_FRAME_SIZE = "FftStream::size";        // :21
class FftStream : public Block {
    detail::Handle h_;
    size_t size_;
    ReadStream<Complex> src_;
    WriteStream<Complex> dst_;
public:
    FftStream(rr_block* h, size_t size, ReadStream<Complex> src, WriteStream<Complex> dst)
        : h_(h), size_(size), src_(std::move(src)), dst_(std::move(dst)) {}
    static std::pair<std::unique_ptr<FftStream>, ReadStream<Complex>> new_(ReadStream<Complex> src, size_t size) {   // :40-60
        auto [w, r] = new_stream<Complex>();
        if (size > w.free()) throw Error("FFT size must be no bigger than stream size");
        return {std::make_unique<FftStream>(rr_fftstream_create(size), size, std::move(src), std::move(w)), std::move(r)};
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {                    // :71-117 — input tags dropped, frame tags added
        auto [input, tags] = src_.read_buf();
        (void)tags;
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        if (w.st == RR_WAIT_SRC) { out.produce(0, {}); return BlockRet::wait(src_.wait_handle(), w.need); }
        if (w.st == RR_WAIT_DST) { out.produce(0, {}); return BlockRet::wait(dst_.wait_handle(), w.need); }
        std::vector<Tag> ft;                      // :98-111
        ft.reserve(w.produced / size_ * 3);
        for (size_t pos = 0; pos < w.produced; pos += size_) {
            ft.emplace_back(pos, TAG_FRAME_SIZE, (uint64_t)size_);
            ft.emplace_back(pos, TAG_FRAME, true);
            ft.emplace_back(pos + size_ - 1, TAG_FRAME, false);
        }
        input.consume(w.consumed);
        out.produce(w.produced, ft);
        return BlockRet::again();
    }
};

// ---- Fft (src/fft.rs:19-56): the message (PDU) form; process() is what work() does to each popped message ---------------------
class Fft {
    detail::Handle h_;
    size_t size_;
    static rr_block* make(size_t size) {
        if (!size) throw Error("FFT called with size 0");                                        // :24-26
        return rr_fftstream_create(size);
    }
public:
    explicit Fft(size_t size) : h_(make(size)), size_(size) {}
    std::vector<Complex> process(const std::vector<Complex>& msg) {                              // :41-55
        std::vector<Complex> out(msg.size());
        Complex dummy{};
        if (rr_fft_process(h_.h, reinterpret_cast<const rr_c32*>(msg.empty() ? &dummy : msg.data()), msg.size(),
                           reinterpret_cast<rr_c32*>(msg.empty() ? &dummy : out.data())) != 0)
            throw Error(rr_last_error());                                                        // "FFT expected {} samples, got {}"
        return out;
    }
    size_t size() const { return size_; }
};

// ---- Wpcr (src/wpcr.rs:84-239): the message (PDU) form; process_one() is what work() does to each popped Vec<Float> -------------
// (rr_wpcr_create / rr_wpcr_process / rr_wpcr_results).  process() takes a batch of bursts in ONE call; `mids`, when given, holds
// Midpointer's offset per burst (wpcr.rs:75-78) instead of a rewritten burst.  The symbols are picked by the drift-free clock of
// include/rustradio_amd.h, not by the reference's f32 accumulator.
class Wpcr {
    detail::Handle h_;
    std::optional<Float> samp_rate_;
public:
    using Packet = std::pair<std::vector<Float>, std::vector<Tag>>;
    explicit Wpcr(std::optional<Float> samp_rate = std::nullopt)                                   // WpcrBuilder::samp_rate (:91-96)
        : h_(rr_wpcr_create(samp_rate ? *samp_rate : std::numeric_limits<Float>::quiet_NaN())), samp_rate_(samp_rate) {}
    std::vector<std::optional<Packet>> process(const std::vector<std::vector<Float>>& bursts, const std::vector<Float>* mids = nullptr) {
        if (mids && mids->size() != bursts.size()) throw Error("Wpcr: one mid per burst");
        std::vector<size_t> starts(bursts.size()), lens(bursts.size());
        size_t total = 0;
        for (size_t b = 0; b < bursts.size(); b++) { starts[b] = total; lens[b] = bursts[b].size(); total += lens[b]; }
        std::vector<Float> x(total + 1), syms(total + 1);
        for (size_t b = 0; b < bursts.size(); b++) std::copy(bursts[b].begin(), bursts[b].end(), x.begin() + (long)starts[b]);
        if (rr_wpcr_process(h_.h, x.data(), total, starts.data(), lens.data(), mids ? mids->data() : nullptr, bursts.size(), syms.data()) != 0)
            throw Error(rr_last_error());
        std::vector<rr_wpcr_result> res(bursts.size() + 1);
        size_t n = 0;
        if (rr_wpcr_results(h_.h, res.data(), bursts.size(), &n) != 0) throw Error(rr_last_error());
        if (n != bursts.size()) throw Error("Wpcr: result count");
        std::vector<std::optional<Packet>> out(bursts.size());
        for (size_t b = 0; b < bursts.size(); b++) {
            const rr_wpcr_result& r = res[b];
            if (!r.ok) continue;                                                                  // None (:159-162): nothing is pushed
            std::vector<Tag> tags{Tag(0, "sps", r.sps), Tag(0, "phase", r.phase)};                // :187-190
            if (samp_rate_) tags.emplace_back(0, "frequency", r.frequency);                       // :191-194
            out[b] = Packet(std::vector<Float>(syms.begin() + (long)starts[b], syms.begin() + (long)(starts[b] + r.nsyms)), std::move(tags));
        }
        return out;
    }
    std::optional<Packet> process_one(const std::vector<Float>& samples) { return process({samples})[0]; }   // :130-197
};

// ---- FcsAdder -> HdlcFramer -> PduToStream<u8> -> [Scrambler::g3ruh] -> [NrziEncode] -> [Map] (src/hdlc_framer.rs:28-86,
// src/pdu_to_stream.rs:57-101, examples/g3ruh.rs:250-267): the message (PDU) form ---------------------------------------------------
// (rr_hdlc_framer_create / rr_hdlc_framer_push / rr_hdlc_framer_records).  push() takes a batch of packets in ONE call and
// returns what the stream behind PduToStream (and the line stages the flags name) receives for them: the frames back to back,
// with a `start` tag carrying U64(len) at each frame's first element (pdu_to_stream.rs:84-92).  The scrambler's register and
// the NRZI level stay in the block from push to push.  T = uint8_t without RR_FRAME_SYMBOLS, Float with it.
template <class T> class HdlcFramer {
    static_assert(std::is_same<T, uint8_t>::value || std::is_same<T, Float>::value, "bits or levels");
    detail::Handle h_;
public:
    struct Frames {
        std::vector<T> stream;
        std::vector<rr_frame_record> records;
        std::vector<Tag> tags;
    };
    explicit HdlcFramer(int flags, Float lo = -1.0f, Float hi = 1.0f)
        : h_(rr_hdlc_framer_create(std::is_same<T, Float>::value ? flags | RR_FRAME_SYMBOLS : flags & ~RR_FRAME_SYMBOLS, lo, hi)) {}
    Frames push(const std::vector<std::vector<uint8_t>>& packets) {
        std::vector<size_t> starts(packets.size() + 1), lens(packets.size() + 1);
        size_t total = 0;
        for (size_t p = 0; p < packets.size(); p++) { starts[p] = total; lens[p] = packets[p].size(); total += lens[p]; }
        std::vector<uint8_t> x(total + 1);
        for (size_t p = 0; p < packets.size(); p++) std::copy(packets[p].begin(), packets[p].end(), x.begin() + (long)starts[p]);
        const size_t cap = rr_hdlc_framer_bound(h_.h, lens.data(), packets.size());
        Frames f;
        f.stream.resize(cap + 1);
        size_t produced = 0;
        if (rr_hdlc_framer_push(h_.h, x.data(), total, starts.data(), lens.data(), packets.size(), f.stream.data(), cap, &produced) != 0)
            throw Error(rr_last_error());
        f.stream.resize(produced);
        f.records.resize(packets.size() + 1);
        size_t n = 0, again = 0;
        if (rr_hdlc_framer_records(h_.h, f.records.data(), packets.size(), &n, &again) != 0) throw Error(rr_last_error());
        if (n != packets.size() || again != produced) throw Error("HdlcFramer: record count");
        f.records.resize(n);
        for (const rr_frame_record& r : f.records) f.tags.emplace_back(r.start, "start", (uint64_t)r.len);
        return f;
    }
    size_t tile_bits() const {
        size_t t = 0;
        if (rr_hdlc_framer_dims(h_.h, &t) != 0) throw Error(rr_last_error());
        return t;
    }
};

// ---- BurstTagger -> StreamToPdu -> [Midpointer] (src/burst_tagger.rs:68-85, src/stream_to_pdu.rs:198-275, src/wpcr.rs:44-82) -----------
// (rr_stream_to_pdu_create / rr_stream_to_pdu_push / rr_pdu_records / rr_pdu_fetch).  push() takes one window of the data stream
// and of the trigger stream and returns what StreamToPdu's output would receive for it: the PDUs this window completes, a burst
// begun in an earlier window whole.  With `midpoint` a Pdu also carries Midpointer's offset (`mid` empty: Midpointer pushes
// nothing for it); centred() is the Vec<Float> Midpointer would push.  The block keeps the open burst: no window is kept here.
class StreamToPdu {
    detail::Handle h_;
    bool midpoint_;
public:
    struct Pdu {
        unsigned long long stream_pos;                // absolute position of the first sample in the data stream
        std::vector<Float> samples;
        std::optional<Float> mid;                     // Midpointer's offset (wpcr.rs:75)
        std::vector<Float> centred() const {          // wpcr.rs:77-78
            std::vector<Float> v(samples);
            if (mid) for (auto& t : v) t -= *mid;
            return v;
        }
    };
    StreamToPdu(Float threshold, size_t max_size, size_t tail, bool midpoint = false)
        : h_(rr_stream_to_pdu_create(threshold, max_size, tail, midpoint ? RR_PDU_MIDPOINT : 0)), midpoint_(midpoint) {}
    rr_block* handle() const { return h_.h; }
    std::vector<Pdu> push(const std::vector<Float>& data, const std::vector<Float>& trigger) {
        if (data.size() != trigger.size()) throw Error("StreamToPdu: data and trigger must have one length");
        if (rr_stream_to_pdu_push(h_.h, data.data(), trigger.data(), data.size()) != 0) throw Error(rr_last_error());
        size_t n = 0;
        if (rr_pdu_records(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_pdu_record> rec(n + 1);
        if (n && rr_pdu_records(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        std::vector<Pdu> out(n);
        for (size_t i = 0; i < n; i++) {
            out[i].stream_pos = rec[i].stream_pos;
            out[i].samples.resize(rec[i].len);
            if (rr_pdu_fetch(h_.h, i, out[i].samples.data(), rec[i].len) != 0) throw Error(rr_last_error());
            if (midpoint_ && rec[i].ok) out[i].mid = rec[i].mid;
        }
        return out;
    }
    // the tags BurstTagger pushed in the most recent window: (window-relative position, value)
    std::vector<std::pair<size_t, bool>> edges() {
        size_t n = 0;
        if (rr_pdu_edges(h_.h, nullptr, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<size_t> pos(n + 1);
        std::vector<unsigned char> val(n + 1);
        if (n && rr_pdu_edges(h_.h, pos.data(), val.data(), n, &n) != 0) throw Error(rr_last_error());
        std::vector<std::pair<size_t, bool>> out(n);
        for (size_t i = 0; i < n; i++) out[i] = {pos[i], val[i] != 0};
        return out;
    }
};

// ---- The sample-rate path of examples/burst_saver.rs:111-131 (rr_burst_saver_create / rr_burst_saver_push / rr_pdu_records /
// rr_pdu_fetch_c32): Tee -> [ComplexToMag2 -> SinglePoleIirFilter(alpha)] and [Delay(delay)] -> BurstTagger(threshold) ->
// StreamToPdu<Complex>(max_size, tail).  push() takes one window of the Complex stream and returns what StreamToPdu's output
// would receive for it; stream_pos counts positions of the delayed stream.  The block keeps the envelope's state, Delay's
// history and the open burst.
class BurstSaver {
    detail::Handle h_;
public:
    struct Pdu {
        unsigned long long stream_pos;
        std::vector<Complex> samples;
    };
    BurstSaver(Float alpha, Float threshold, size_t delay, size_t max_size, size_t tail)
        : h_(rr_burst_saver_create(alpha, threshold, delay, max_size, tail)) {}
    rr_block* handle() const { return h_.h; }
    // envelope: when given, receives the filtered power of the window (what the trigger branch carries)
    std::vector<Pdu> push(const std::vector<Complex>& window, std::vector<Float>* envelope = nullptr) {
        if (envelope) envelope->assign(window.size(), 0.0f);
        if (rr_burst_saver_push(h_.h, reinterpret_cast<const rr_c32*>(window.data()), window.size(),
                                envelope && !window.empty() ? envelope->data() : nullptr) != 0)
            throw Error(rr_last_error());
        size_t n = 0;
        if (rr_pdu_records(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_pdu_record> rec(n + 1);
        if (n && rr_pdu_records(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        std::vector<Pdu> out(n);
        for (size_t i = 0; i < n; i++) {
            out[i].stream_pos = rec[i].stream_pos;
            out[i].samples.resize(rec[i].len);
            if (rr_pdu_fetch_c32(h_.h, i, reinterpret_cast<rr_c32*>(out[i].samples.data()), rec[i].len) != 0) throw Error(rr_last_error());
        }
        return out;
    }
};

// ---- HdlcDeframer (src/hdlc_deframer.rs:80-232): the message (PDU) form of its output -------------------------------------------------
// (rr_hdlc_deframer_create / rr_hdlc_deframer_push / rr_hdlc_frames / rr_hdlc_frame_bytes / rr_hdlc_stats).  push() takes the next
// bits of the stream, one per byte, and returns what the NCWriteStream<Vec<u8>> behind the block receives for them: one
// (bytes, tags) per frame whose closing flag ended inside them, each with the `packet_pos` tag (:193).  The machine, the open
// gap's bits and the counters stay in the block from push to push; output_space (:237-253) has no counterpart.
class HdlcDeframer {
    detail::Handle h_;
public:
    using Packet = std::pair<std::vector<uint8_t>, std::vector<Tag>>;
    struct Stats { unsigned long long decoded, crc_error, bitfixed; };
    HdlcDeframer(size_t min_size, size_t max_size, bool keep_checksum = false, bool fix_bits = false)
        : h_(rr_hdlc_deframer_create(min_size, max_size, (keep_checksum ? RR_HDLC_KEEP_CHECKSUM : 0) | (fix_bits ? RR_HDLC_FIX_BITS : 0))) {}
    rr_block* handle() const { return h_.h; }
    std::vector<Packet> push(const std::vector<uint8_t>& bits, std::vector<bool>* repaired = nullptr) {
        if (rr_hdlc_deframer_push(h_.h, bits.data(), bits.size()) != 0) throw Error(rr_last_error());
        size_t n = 0, nb = 0;
        if (rr_hdlc_frames(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_hdlc_frame> rec(n + 1);
        if (n && rr_hdlc_frames(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        if (rr_hdlc_frame_bytes(h_.h, nullptr, 0, &nb) != 0) throw Error(rr_last_error());
        std::vector<uint8_t> arena(nb + 1);
        if (n && nb && rr_hdlc_frame_bytes(h_.h, arena.data(), nb, &nb) != 0) throw Error(rr_last_error());
        std::vector<Packet> out(n);
        if (repaired) repaired->assign(n, false);
        for (size_t i = 0; i < n; i++) {
            if (rec[i].start > nb || rec[i].len > nb - rec[i].start) throw Error("HdlcDeframer: frame outside the arena");
            out[i].first.assign(arena.begin() + (long)rec[i].start, arena.begin() + (long)(rec[i].start + rec[i].len));
            out[i].second.emplace_back(0, "packet_pos", (uint64_t)rec[i].pos);
            if (repaired) (*repaired)[i] = (rec[i].flags & 1u) != 0;
        }
        return out;
    }
    Stats stats() {
        Stats s{0, 0, 0};
        if (rr_hdlc_stats(h_.h, &s.decoded, &s.crc_error, &s.bitfixed) != 0) throw Error(rr_last_error());
        return s;
    }
    size_t carry_bits() const {
        size_t t = 0, c = 0;
        if (rr_hdlc_deframer_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error());
        return c;
    }
};

// ---- KissFrame -> KissDecode (src/kiss.rs:96-228): the message (PDU) form of its output --------------------------------------------------
// (rr_kiss_decode_create / rr_kiss_decode_push / rr_kiss_packets / rr_kiss_packet_bytes / rr_kiss_decode_stats).  push() takes the
// next bytes of the KISS stream and returns what the NCWriteStream<Vec<u8>> behind KissDecode receives for them: one (bytes, tags)
// per packet whose closing FEND lay inside them, each with the three tags of :122-134.  Whether a FEND has been seen, the open
// gap's bytes and the counters stay in the block from push to push; dst.remaining() (:99-101) has no counterpart.
class KissDecode {
    detail::Handle h_;
public:
    using Packet = std::pair<std::vector<uint8_t>, std::vector<Tag>>;
    struct Stats { unsigned long long frames, delivered, nondata, bad_escape, overlong; };
    explicit KissDecode(size_t max_len = 10000) : h_(rr_kiss_decode_create(max_len)) {}
    rr_block* handle() const { return h_.h; }
    std::vector<Packet> push(const std::vector<uint8_t>& bytes, std::vector<uint64_t>* pos = nullptr) {
        if (rr_kiss_decode_push(h_.h, bytes.data(), bytes.size()) != 0) throw Error(rr_last_error());
        size_t n = 0, nb = 0;
        if (rr_kiss_packets(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_kiss_packet> rec(n + 1);
        if (n && rr_kiss_packets(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        if (rr_kiss_packet_bytes(h_.h, nullptr, 0, &nb) != 0) throw Error(rr_last_error());
        std::vector<uint8_t> arena(nb + 1);
        if (n && nb && rr_kiss_packet_bytes(h_.h, arena.data(), nb, &nb) != 0) throw Error(rr_last_error());
        std::vector<Packet> out(n);
        if (pos) pos->assign(n, 0);
        for (size_t i = 0; i < n; i++) {
            if (rec[i].start > nb || rec[i].len > nb - rec[i].start) throw Error("KissDecode: packet outside the arena");
            out[i].first.assign(arena.begin() + (long)rec[i].start, arena.begin() + (long)(rec[i].start + rec[i].len));
            out[i].second.emplace_back(0, "KissDecode:port", (uint64_t)rec[i].port);
            out[i].second.emplace_back(0, "KissDecode:input-bytes", (uint64_t)rec[i].in_bytes);
            out[i].second.emplace_back(0, "KissDecode:output-bytes", (uint64_t)rec[i].len);
            if (pos) (*pos)[i] = rec[i].pos;
        }
        return out;
    }
    Stats stats() {
        unsigned long long s[5] = {0, 0, 0, 0, 0};
        if (rr_kiss_decode_stats(h_.h, s) != 0) throw Error(rr_last_error());
        return Stats{s[0], s[1], s[2], s[3], s[4]};
    }
    size_t carry_bytes() const {
        size_t t = 0, c = 0, k = 0;
        if (rr_kiss_decode_dims(h_.h, &t, &c, &k) != 0) throw Error(rr_last_error());
        return c;
    }
};

// ---- KissEncode -> PduToStream<u8> (src/kiss.rs:247-286, src/pdu_to_stream.rs:57-101) ---------------------------------------------------
// (rr_kiss_encode_create / rr_kiss_encode_bound / rr_kiss_encode_push / rr_kiss_encode_records).  push() takes what the chain pops
// in one go, every packet with its "KissEncode:port" (none: 0; 16 or more: 0), and returns the frames back to back with their
// records.  The port byte is not escaped, as in the reference.
class KissEncode {
    detail::Handle h_;
public:
    struct Frames {
        std::vector<uint8_t> stream;
        std::vector<rr_kiss_frame_record> records;
    };
    KissEncode() : h_(rr_kiss_encode_create()) {}
    rr_block* handle() const { return h_.h; }
    Frames push(const std::vector<std::vector<uint8_t>>& packets, const std::vector<unsigned>& ports = {}) {
        if (!ports.empty() && ports.size() != packets.size()) throw Error("KissEncode: one port per packet");
        std::vector<size_t> starts(packets.size() + 1), lens(packets.size() + 1);
        size_t total = 0;
        for (size_t p = 0; p < packets.size(); p++) { starts[p] = total; lens[p] = packets[p].size(); total += lens[p]; }
        std::vector<uint8_t> x(total + 1);
        for (size_t p = 0; p < packets.size(); p++) std::copy(packets[p].begin(), packets[p].end(), x.begin() + (long)starts[p]);
        const size_t cap = rr_kiss_encode_bound(lens.data(), packets.size());
        Frames f;
        f.stream.resize(cap + 1);
        size_t produced = 0;
        if (rr_kiss_encode_push(h_.h, x.data(), total, starts.data(), lens.data(), ports.empty() ? nullptr : ports.data(), packets.size(),
                                f.stream.data(), cap, &produced) != 0)
            throw Error(rr_last_error());
        f.stream.resize(produced);
        f.records.resize(packets.size() + 1);
        size_t n = 0, again = 0;
        if (rr_kiss_encode_records(h_.h, f.records.data(), packets.size(), &n, &again) != 0) throw Error(rr_last_error());
        if (n != packets.size() || again != produced) throw Error("KissEncode: record count");
        f.records.resize(n);
        return f;
    }
};

// ---- PwmDecoder (src/pwm_decoder.rs:165-266, 385-513): the builder and the frames of its NCWriteStream<PwmFrame> ------------------------
// (rr_pwm_decoder_create / rr_pwm_decoder_push / rr_pwm_decoder_flush / rr_pwm_frames / rr_pwm_frame_bits).  The builder holds the
// reference's defaults (:76-98) and build<T>() refuses what validate() refuses, in its words.  push() takes the next samples of the
// power stream (T = Float) or of the Complex stream in front of ComplexToMag2 (T = Complex, examples/restaurant_pager.rs) and
// returns the frames of every transmission whose reset sample lies inside them; finish() is EOF.  The slicer, the open frame and
// the candidates stay in the block from push to push; the pending queue's back-pressure (:602-610) has no counterpart.
enum class PwmGapPulse { Data, Delimiter };
struct PwmFrame {
    std::vector<uint8_t> bits_;
    size_t repeats_ = 0;
    uint64_t first_sample_ = 0;
    const std::vector<uint8_t>& bits() const { return bits_; }
    size_t repeats() const { return repeats_; }
    uint64_t first_sample() const { return first_sample_; }
    size_t len() const { return bits_.size(); }
    bool is_empty() const { return bits_.empty(); }
};
template <class T> class PwmDecoder;
class PwmDecoderBuilder {
    float high_, low_;
    size_t short_, long_, tol_, fgap_, rgap_, frame_bits_ = 0, max_frame_bits_ = 4096, max_distinct_ = 256, min_repeats_ = 1;
    bool fixed_ = false, short_is_one_ = true;
    PwmGapPulse gap_pulse_ = PwmGapPulse::Data;
    template <class T> friend class PwmDecoder;
public:
    PwmDecoderBuilder(float high_threshold, size_t short_width, size_t long_width, size_t frame_gap, size_t reset_gap)
        : high_(high_threshold), low_(high_threshold / 2.0f), short_(short_width), long_(long_width),
          tol_((long_width > short_width ? long_width - short_width : short_width - long_width) / 2), fgap_(frame_gap), rgap_(reset_gap) {}
    PwmDecoderBuilder& low_threshold(float v) { low_ = v; return *this; }
    PwmDecoderBuilder& pulse_tolerance(size_t v) { tol_ = v; return *this; }
    PwmDecoderBuilder& frame_bits(size_t bits) { fixed_ = true; frame_bits_ = bits; return *this; }      // Some(bits)
    PwmDecoderBuilder& any_frame_bits() { fixed_ = false; frame_bits_ = 0; return *this; }               // None
    PwmDecoderBuilder& max_frame_bits(size_t v) { max_frame_bits_ = v; return *this; }
    PwmDecoderBuilder& max_distinct_frames(size_t v) { max_distinct_ = v; return *this; }
    PwmDecoderBuilder& min_repeats(size_t v) { min_repeats_ = v; return *this; }
    PwmDecoderBuilder& short_is_one(bool v) { short_is_one_ = v; return *this; }
    PwmDecoderBuilder& gap_pulse(PwmGapPulse v) { gap_pulse_ = v; return *this; }
    template <class T = Float> PwmDecoder<T> build() const { return PwmDecoder<T>(*this); }
};
template <class T = Float> class PwmDecoder {
    static_assert(std::is_same<T, Float>::value || std::is_same<T, Complex>::value, "PwmDecoder: Float (power) or Complex samples");
    detail::Handle h_;
    static rr_block* make(const PwmDecoderBuilder& b) {
        // Some(0) cannot cross the C ABI (0 is None): validate()'s own refusal (:133-137)
        if (b.fixed_ && b.frame_bits_ == 0) throw Error("PwmDecoder fixed frame length must be greater than zero");
        return rr_pwm_decoder_create(b.high_, b.low_, b.short_, b.long_, b.tol_, b.fgap_, b.rgap_, b.fixed_ ? b.frame_bits_ : 0, b.max_frame_bits_,
                                     b.max_distinct_, b.min_repeats_,
                                     (b.short_is_one_ ? 0 : RR_PWM_SHORT_IS_ZERO) | (b.gap_pulse_ == PwmGapPulse::Delimiter ? RR_PWM_GAP_DELIMITER : 0),
                                     sizeof(T));
    }
    std::vector<PwmFrame> fetch() {
        size_t n = 0, nb = 0;
        if (rr_pwm_frames(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_pwm_frame> rec(n + 1);
        if (n && rr_pwm_frames(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        if (rr_pwm_frame_bits(h_.h, nullptr, 0, &nb) != 0) throw Error(rr_last_error());
        std::vector<uint8_t> arena(nb + 1);
        if (n && nb && rr_pwm_frame_bits(h_.h, arena.data(), nb, &nb) != 0) throw Error(rr_last_error());
        std::vector<PwmFrame> out(n);
        for (size_t i = 0; i < n; i++) {
            if (rec[i].start > nb || rec[i].len > nb - rec[i].start) throw Error("PwmDecoder: frame outside the arena");
            out[i].bits_.assign(arena.begin() + (long)rec[i].start, arena.begin() + (long)(rec[i].start + rec[i].len));
            out[i].repeats_ = rec[i].repeats;
            out[i].first_sample_ = rec[i].first_sample;
        }
        return out;
    }
public:
    static PwmDecoderBuilder builder(float high_threshold, size_t short_width, size_t long_width, size_t frame_gap, size_t reset_gap) {
        return PwmDecoderBuilder(high_threshold, short_width, long_width, frame_gap, reset_gap);
    }
    explicit PwmDecoder(const PwmDecoderBuilder& b) : h_(make(b)) {}
    rr_block* handle() const { return h_.h; }
    std::vector<PwmFrame> push(const std::vector<T>& samples) {
        if (rr_pwm_decoder_push(h_.h, samples.data(), samples.size()) != 0) throw Error(rr_last_error());
        return fetch();
    }
    std::vector<PwmFrame> finish() {
        if (rr_pwm_decoder_flush(h_.h, nullptr) != 0) throw Error(rr_last_error());
        return fetch();
    }
    size_t tile_samples() const {
        size_t t = 0;
        if (rr_pwm_decoder_dims(h_.h, &t) != 0) throw Error(rr_last_error());
        return t;
    }
};

// ---- SymbolSync (src/symbol_sync.rs:46-217) x nstreams: the window form of its streams ---------------------------------------------
// (rr_symbol_sync_create / rr_symbol_sync_push / rr_symbol_sync_push_dev / rr_symbol_sync_produced).  push() takes the next samples
// of every stream and returns what the block's dst (and out_clock(), when asked for) receive for them; each stream's clock state
// stays in the block from push to push.  The output always has room, so the `opos == olen` break (:150-152) has no counterpart.
class SymbolSync {
    detail::Handle h_;
    size_t nstreams_;
public:
    struct Output { std::vector<std::vector<float>> symbols, clock; };      // one vector per stream; clock empty unless asked for
    SymbolSync(float sps, float max_deviation, const std::vector<float>& taps, size_t nstreams = 1)
        : h_(rr_symbol_sync_create(sps, max_deviation, taps.data(), taps.size(), nstreams)), nstreams_(nstreams) {}
    rr_block* handle() const { return h_.h; }
    size_t nstreams() const { return nstreams_; }
    // rows[c] = the next samples of stream c, all of one length
    Output push(const std::vector<std::vector<float>>& rows, bool want_clock = false) {
        if (rows.size() != nstreams_) throw Error("SymbolSync: one row per stream");
        const size_t n = rows.empty() ? 0 : rows[0].size();
        std::vector<float> in(nstreams_ * n + 1), syms(nstreams_ * n + 1), clk(want_clock ? nstreams_ * n + 1 : 1);
        for (size_t c = 0; c < nstreams_; c++) {
            if (rows[c].size() != n) throw Error("SymbolSync: rows of one length");
            std::copy(rows[c].begin(), rows[c].end(), in.begin() + (long)(c * n));
        }
        std::vector<size_t> produced(nstreams_);
        if (rr_symbol_sync_push(h_.h, in.data(), n, n, syms.data(), want_clock ? clk.data() : nullptr, n, produced.data()) != 0)
            throw Error(rr_last_error());
        Output out;
        out.symbols.resize(nstreams_);
        if (want_clock) out.clock.resize(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) {
            const size_t k = std::min(produced[c], n);
            out.symbols[c].assign(syms.begin() + (long)(c * n), syms.begin() + (long)(c * n + k));
            if (want_clock) out.clock[c].assign(clk.begin() + (long)(c * n), clk.begin() + (long)(c * n + k));
        }
        return out;
    }
    // device windows in the layout of rr_fm_multi_create's output; asynchronous on hip_stream, produced() waits
    void push_dev(const void* d_in, size_t in_stride, size_t n, void* d_syms, void* d_clock, size_t out_stride, void* hip_stream = nullptr) {
        if (rr_symbol_sync_push_dev(h_.h, d_in, in_stride, n, d_syms, d_clock, out_stride, hip_stream) != 0) throw Error(rr_last_error());
    }
    std::vector<size_t> produced() {
        std::vector<size_t> k(nstreams_);
        size_t total = 0;
        if (rr_symbol_sync_produced(h_.h, k.data(), k.size(), &total) != 0) throw Error(rr_last_error());
        return k;
    }
    const void* counts_dev() { return rr_symbol_sync_counts_dev(h_.h); }
};

// ---- BinarySlicer -> [XorConst(1)] -> [NrziDecode] -> [Descrambler] -> HdlcDeframer x nstreams: the consumer of SymbolSync ----------
// (rr_hdlc_receiver_create / _push / _push_dev / _frames / _frame_bytes / _stats / _consumed).  push() takes the next symbols of
// every stream (rows of any lengths) and returns, per stream, what HdlcDeframer's dst receives for them; push_dev() takes
// SymbolSync's device windows and counts_dev() as they are.  Every stream's state stays in the block from push to push.
class HdlcReceiver {
    detail::Handle h_;
    size_t nstreams_;
public:
    using Packet = HdlcDeframer::Packet;
    using Stats = HdlcDeframer::Stats;
    // bit_flags: RR_BITS_*; mask, seed, len: Descrambler::new's (read with RR_BITS_DESCRAMBLE only)
    HdlcReceiver(size_t nstreams, int bit_flags, unsigned long long mask, unsigned long long seed, unsigned len, size_t min_size,
                 size_t max_size, bool keep_checksum = false, bool fix_bits = false)
        : h_(rr_hdlc_receiver_create(nstreams, bit_flags, mask, seed, len, min_size, max_size,
                                     (keep_checksum ? RR_HDLC_KEEP_CHECKSUM : 0) | (fix_bits ? RR_HDLC_FIX_BITS : 0))),
          nstreams_(nstreams) {}
    rr_block* handle() const { return h_.h; }
    size_t nstreams() const { return nstreams_; }
    // the frames of the most recent push, per stream, in stream order (waits for it)
    std::vector<std::vector<Packet>> packets(std::vector<std::vector<bool>>* repaired = nullptr) {
        size_t n = 0, nb = 0;
        if (rr_hdlc_receiver_frames(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_hdlc_stream_frame> rec(n + 1);
        if (n && rr_hdlc_receiver_frames(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        if (rr_hdlc_receiver_frame_bytes(h_.h, nullptr, 0, &nb) != 0) throw Error(rr_last_error());
        std::vector<uint8_t> arena(nb + 1);
        if (n && nb && rr_hdlc_receiver_frame_bytes(h_.h, arena.data(), nb, &nb) != 0) throw Error(rr_last_error());
        std::vector<std::vector<Packet>> out(nstreams_);
        if (repaired) repaired->assign(nstreams_, {});
        for (size_t i = 0; i < n; i++) {
            if (rec[i].stream >= nstreams_) throw Error("HdlcReceiver: no such stream");
            if (rec[i].start > nb || rec[i].len > nb - rec[i].start) throw Error("HdlcReceiver: frame outside the arena");
            Packet p;
            p.first.assign(arena.begin() + (long)rec[i].start, arena.begin() + (long)(rec[i].start + rec[i].len));
            p.second.emplace_back(0, "packet_pos", (uint64_t)rec[i].pos);
            out[rec[i].stream].push_back(std::move(p));
            if (repaired) (*repaired)[rec[i].stream].push_back((rec[i].flags & 1u) != 0);
        }
        return out;
    }
    // rows[c] = the next symbols of stream c
    std::vector<std::vector<Packet>> push(const std::vector<std::vector<float>>& rows, std::vector<std::vector<bool>>* repaired = nullptr) {
        if (rows.size() != nstreams_) throw Error("HdlcReceiver: one row per stream");
        size_t n_cap = 0;
        for (auto& r : rows) n_cap = std::max(n_cap, r.size());
        std::vector<float> in(nstreams_ * n_cap + 1);
        std::vector<size_t> counts(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) {
            std::copy(rows[c].begin(), rows[c].end(), in.begin() + (long)(c * n_cap));
            counts[c] = rows[c].size();
        }
        if (rr_hdlc_receiver_push(h_.h, in.data(), n_cap, n_cap, counts.data()) != 0) throw Error(rr_last_error());
        return packets(repaired);
    }
    // device windows in the layout SymbolSync::push_dev writes, d_counts = SymbolSync::counts_dev() (or null: n_cap each);
    // asynchronous on hip_stream, packets() waits
    void push_dev(const void* d_syms, size_t stride, size_t n_cap, const void* d_counts, void* hip_stream = nullptr) {
        if (rr_hdlc_receiver_push_dev(h_.h, d_syms, stride, n_cap, d_counts, hip_stream) != 0) throw Error(rr_last_error());
    }
    std::vector<Stats> stats() {
        std::vector<unsigned long long> d(nstreams_), e(nstreams_), f(nstreams_);
        size_t total = 0;
        if (rr_hdlc_receiver_stats(h_.h, d.data(), e.data(), f.data(), nstreams_, &total) != 0) throw Error(rr_last_error());
        std::vector<Stats> out(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) out[c] = Stats{d[c], e[c], f[c]};
        return out;
    }
    std::vector<unsigned long long> consumed() {
        std::vector<unsigned long long> k(nstreams_);
        size_t total = 0;
        if (rr_hdlc_receiver_consumed(h_.h, k.data(), k.size(), &total) != 0) throw Error(rr_last_error());
        return k;
    }
    size_t carry_bits() const {
        size_t t = 0, c = 0;
        if (rr_hdlc_receiver_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error());
        return c;
    }
};

// ---- BinarySlicer -> [XorConst(1)] -> CorrelateAccessCodeTag(il2p SYNC_WORD) -> Il2pDeframer x nstreams (examples/il2p-1200-rx.rs:118-137)
// (rr_il2p_receiver_create / _push / _push_dev / _headers / _stats / _consumed / _dims).  push() takes the next symbols of every
// stream (rows of any lengths) and returns the headers whose 120th bit lay in them, ascending by (stream, pos); push_dev() takes
// SymbolSync's device windows and counts_dev() as they are.  Every stream's state stays in the block from push to push.
class Il2pReceiver {
    detail::Handle h_;
    size_t nstreams_;
public:
    struct Stats { unsigned long long headers, syncs; };
    Il2pReceiver(size_t nstreams, bool invert = false, size_t allowed_diffs = 0)
        : h_(rr_il2p_receiver_create(nstreams, invert ? RR_BITS_INVERT : 0, allowed_diffs)), nstreams_(nstreams) {}
    rr_block* handle() const { return h_.h; }
    size_t nstreams() const { return nstreams_; }
    // the headers of the most recent push (waits for it)
    std::vector<rr_il2p_header> headers() {
        size_t n = 0;
        if (rr_il2p_receiver_headers(h_.h, nullptr, 0, &n) != 0) throw Error(rr_last_error());
        std::vector<rr_il2p_header> rec(n);
        if (n && rr_il2p_receiver_headers(h_.h, rec.data(), n, &n) != 0) throw Error(rr_last_error());
        rec.resize(std::min(n, rec.size()));
        for (auto& r : rec)
            if (r.stream >= nstreams_) throw Error("Il2pReceiver: no such stream");
        return rec;
    }
    // rows[c] = the next symbols of stream c
    std::vector<rr_il2p_header> push(const std::vector<std::vector<float>>& rows) {
        if (rows.size() != nstreams_) throw Error("Il2pReceiver: one row per stream");
        size_t n_cap = 0;
        for (auto& r : rows) n_cap = std::max(n_cap, r.size());
        std::vector<float> in(nstreams_ * n_cap + 1);
        std::vector<size_t> counts(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) {
            std::copy(rows[c].begin(), rows[c].end(), in.begin() + (long)(c * n_cap));
            counts[c] = rows[c].size();
        }
        if (rr_il2p_receiver_push(h_.h, in.data(), n_cap, n_cap, counts.data()) != 0) throw Error(rr_last_error());
        return headers();
    }
    // device windows in the layout SymbolSync::push_dev writes, d_counts = SymbolSync::counts_dev() (or null: n_cap each);
    // asynchronous on hip_stream, headers() waits
    void push_dev(const void* d_syms, size_t stride, size_t n_cap, const void* d_counts, void* hip_stream = nullptr) {
        if (rr_il2p_receiver_push_dev(h_.h, d_syms, stride, n_cap, d_counts, hip_stream) != 0) throw Error(rr_last_error());
    }
    std::vector<Stats> stats() {
        std::vector<unsigned long long> h(nstreams_), s(nstreams_);
        size_t total = 0;
        if (rr_il2p_receiver_stats(h_.h, h.data(), s.data(), nstreams_, &total) != 0) throw Error(rr_last_error());
        std::vector<Stats> out(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) out[c] = Stats{h[c], s[c]};
        return out;
    }
    std::vector<unsigned long long> consumed() {
        std::vector<unsigned long long> k(nstreams_);
        size_t total = 0;
        if (rr_il2p_receiver_consumed(h_.h, k.data(), k.size(), &total) != 0) throw Error(rr_last_error());
        return k;
    }
    // -> (tile_bits, carry_bits)
    std::pair<size_t, size_t> dims() const {
        size_t t = 0, c = 0;
        if (rr_il2p_receiver_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error());
        return {t, c};
    }
};

// ---- AfskDemod: Hilbert -> QuadratureDemod -> FftFilterFloat -> AddConst (examples/ax25-1200-rx.rs:238-247) x nstreams ------------
// (rr_afsk_demod_create / rr_afsk_demod_push / rr_afsk_demod_push_dev / rr_afsk_demod_dims).  push() takes the next samples of
// every stream and returns the soft samples they complete: one fewer than pushed for the push that starts the streams, as many
// as pushed after it.  Each stream's latest samples stay in the block from push to push.
class AfskDemod {
    detail::Handle h_;
    size_t nstreams_;
public:
    AfskDemod(size_t nstreams, size_t hilbert_ntaps, int window, float window_parm, float gain, const std::vector<float>& taps,
              float offset)
        : h_(rr_afsk_demod_create(nstreams, hilbert_ntaps, window, window_parm, gain, taps.data(), taps.size(), offset)),
          nstreams_(nstreams) {}
    rr_block* handle() const { return h_.h; }
    size_t nstreams() const { return nstreams_; }
    // rows[c] = the next samples of stream c, all of one length -> the outputs of stream c, all of one length
    std::vector<std::vector<float>> push(const std::vector<std::vector<float>>& rows) {
        if (rows.size() != nstreams_) throw Error("AfskDemod: one row per stream");
        const size_t n = rows.empty() ? 0 : rows[0].size();
        std::vector<float> in(nstreams_ * n + 1), out(nstreams_ * n + 1);
        for (size_t c = 0; c < nstreams_; c++) {
            if (rows[c].size() != n) throw Error("AfskDemod: rows of one length");
            std::copy(rows[c].begin(), rows[c].end(), in.begin() + (long)(c * n));
        }
        size_t produced = 0;
        if (rr_afsk_demod_push(h_.h, in.data(), n, n, out.data(), n, &produced) != 0) throw Error(rr_last_error());
        produced = std::min(produced, n);
        std::vector<std::vector<float>> res(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) res[c].assign(out.begin() + (long)(c * n), out.begin() + (long)(c * n + produced));
        return res;
    }
    // device windows in the layout of rr_fm_multi_create's output; asynchronous on hip_stream -> produced, the n of the
    // following SymbolSync::push_dev
    size_t push_dev(const void* d_in, size_t in_stride, size_t n, void* d_out, size_t out_stride, void* hip_stream = nullptr) {
        size_t produced = 0;
        if (rr_afsk_demod_push_dev(h_.h, d_in, in_stride, n, d_out, out_stride, &produced, hip_stream) != 0) throw Error(rr_last_error());
        return produced;
    }
    size_t tile_samples() const { size_t t = 0, c = 0; if (rr_afsk_demod_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error()); return t; }
    size_t carry_samples() const { size_t t = 0, c = 0; if (rr_afsk_demod_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error()); return c; }
};

// ---- AmDemod: Map(norm) -> FftFilterFloat -> RationalResampler -> MultiplyConst (examples/airspy_am_decode.rs) x nstreams ----------
// (rr_am_demod_create / rr_am_demod_push / rr_am_demod_push_dev / rr_am_demod_dims).  push() takes the next Complex samples of
// every stream and returns the audio samples they complete: ceil(N interp / deci) per stream after N samples in all.  Each
// stream's latest magnitudes stay in the block from push to push.
class AmDemod {
    detail::Handle h_;
    size_t nstreams_, interp_, deci_;
    unsigned long long total_ = 0;
    static size_t gcd_(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }
public:
    AmDemod(size_t nstreams, const std::vector<float>& taps, size_t interp, size_t deci, float scale)
        : h_(rr_am_demod_create(nstreams, taps.data(), taps.size(), interp, deci, scale)), nstreams_(nstreams) {
        const size_t g = gcd_(interp, deci);
        interp_ = interp / g; deci_ = deci / g;
    }
    rr_block* handle() const { return h_.h; }
    size_t nstreams() const { return nstreams_; }
    // outputs of each stream a push of n samples would deliver now
    size_t count(size_t n) const {
        auto up = [&](unsigned long long N) { return (N * interp_ + deci_ - 1) / deci_; };
        return (size_t)(up(total_ + n) - up(total_));
    }
    // rows[c] = the next samples of stream c, all of one length -> the outputs of stream c, all of one length
    std::vector<std::vector<float>> push(const std::vector<std::vector<Complex>>& rows) {
        if (rows.size() != nstreams_) throw Error("AmDemod: one row per stream");
        const size_t n = rows.empty() ? 0 : rows[0].size(), cap = count(n);
        std::vector<Complex> in(nstreams_ * n + 1);
        std::vector<float> out(nstreams_ * cap + 1);
        for (size_t c = 0; c < nstreams_; c++) {
            if (rows[c].size() != n) throw Error("AmDemod: rows of one length");
            std::copy(rows[c].begin(), rows[c].end(), in.begin() + (long)(c * n));
        }
        size_t produced = 0;
        if (rr_am_demod_push(h_.h, reinterpret_cast<const rr_c32*>(in.data()), n, n, out.data(), cap, &produced) != 0) throw Error(rr_last_error());
        total_ += n;
        produced = std::min(produced, cap);
        std::vector<std::vector<float>> res(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) res[c].assign(out.begin() + (long)(c * cap), out.begin() + (long)(c * cap + produced));
        return res;
    }
    // device windows in the layout of rr_channelizer_create's output; asynchronous on hip_stream -> produced
    size_t push_dev(const void* d_in, size_t in_stride, size_t n, void* d_out, size_t out_stride, void* hip_stream = nullptr) {
        size_t produced = 0;
        if (rr_am_demod_push_dev(h_.h, d_in, in_stride, n, d_out, out_stride, &produced, hip_stream) != 0) throw Error(rr_last_error());
        total_ += n;
        return produced;
    }
    size_t tile_outputs() const { size_t t = 0, c = 0; if (rr_am_demod_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error()); return t; }
    size_t carry_samples() const { size_t t = 0, c = 0; if (rr_am_demod_dims(h_.h, &t, &c) != 0) throw Error(rr_last_error()); return c; }
};

// ---- #[rustradio(sync)] blocks: MultiplyConst (src/multiply_const.rs), FastFM (src/quadrature_demod.rs:144-165) ----------
// work() per rustradio_macros_code/src/lib.rs:458-515; a tag at position pos < n passes through at pos.
template <class In, class Out> class SyncBlock : public Block {
protected:
    detail::Handle h_;
    ReadStream<In> src_;
    WriteStream<Out> dst_;
public:
    SyncBlock(rr_block* h, ReadStream<In> src, WriteStream<Out> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)) {}
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        std::vector<Tag> keep;
        for (auto& t : tags) if (t.pos() < w.produced) keep.push_back(t);
        input.consume(w.consumed);
        out.produce(w.produced, keep);
        return w.st == RR_WAIT_DST ? BlockRet::wait(dst_.wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
};
template <class T> class MultiplyConst : public SyncBlock<T, T> {
    static rr_block* make(T val) {
        if constexpr (std::is_same<T, Complex>::value) return rr_multiply_const_c32_create(val.real(), val.imag());
        else return rr_multiply_const_f32_create(val);
    }
public:
    using SyncBlock<T, T>::SyncBlock;
    static std::pair<std::unique_ptr<MultiplyConst<T>>, ReadStream<T>> new_(ReadStream<T> src, T val) {
        auto [w, r] = new_stream<T>();
        return {std::make_unique<MultiplyConst<T>>(make(val), std::move(src), std::move(w)), std::move(r)};
    }
};
// AddConst (src/add_const.rs:51-68): out = in + val, one f32 add per component
template <class T> class AddConst : public SyncBlock<T, T> {
    static rr_block* make(T val) {
        if constexpr (std::is_same<T, Complex>::value) return rr_add_const_c32_create(val.real(), val.imag());
        else return rr_add_const_f32_create(val);
    }
public:
    using SyncBlock<T, T>::SyncBlock;
    static std::pair<std::unique_ptr<AddConst<T>>, ReadStream<T>> new_(ReadStream<T> src, T val) {
        auto [w, r] = new_stream<T>();
        return {std::make_unique<AddConst<T>>(make(val), std::move(src), std::move(w)), std::move(r)};
    }
};
class FastFM : public SyncBlock<Complex, Float> {
public:
    using SyncBlock<Complex, Float>::SyncBlock;
    static std::pair<std::unique_ptr<FastFM>, ReadStream<Float>> new_(ReadStream<Complex> src) {
        auto [w, r] = new_stream<Float>();
        return {std::make_unique<FastFM>(rr_fastfm_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
// Vco (src/vco.rs:9-37), also a sync block: Float -> Complex(sin phase, cos phase), phase += k * a in f64.  `k` crosses the
// C ABI as its IEEE-754 bit pattern (f64::to_bits), so it arrives exactly.
namespace detail {
inline unsigned long long f64_bits(double k) {
    unsigned long long b;
    static_assert(sizeof b == sizeof k, "binary64");
    std::memcpy(&b, &k, sizeof b);
    return b;
}
}  // namespace detail

// ---- FskTx: the modulators of examples/bell202.rs:166-183 (AFSK) and examples/g3ruh.rs:256-272 (DIRECT) in PDU form --------------
// (rr_fsk_tx_create / rr_fsk_tx_count / rr_fsk_tx_push / rr_fsk_tx_push_dev / rr_fsk_tx_dims).  push() takes the next line bits
// (HdlcFramer's u8, nonzero = 1) and returns everything they produce; both phases stay in the block from push to push.
class FskTx {
    detail::Handle h_;
public:
    enum Mode { Direct = RR_FSK_TX_DIRECT, Afsk = RR_FSK_TX_AFSK };
    struct Pushed {
        std::vector<Complex> out;
        std::vector<float> audio;             // AFSK mode with audio asked for: a[] of this push
    };
    FskTx(int mode, size_t interp1, size_t deci1, float lo, float hi, double k1, float gain, size_t interp2 = 1, size_t deci2 = 1,
          double k2 = 0.0)
        : h_(rr_fsk_tx_create(mode, interp1, deci1, lo, hi, detail::f64_bits(k1), gain, interp2, deci2, detail::f64_bits(k2))) {}
    rr_block* handle() const { return h_.h; }
    // (n_audio, n_out) of the NEXT push of n_bits
    std::pair<size_t, size_t> count(size_t n_bits) const {
        size_t a = 0, o = 0;
        if (rr_fsk_tx_count(h_.h, n_bits, &a, &o) != 0) throw Error(rr_last_error());
        return {a, o};
    }
    Pushed push(const std::vector<unsigned char>& bits, bool want_audio = false) {
        const auto [na, no] = count(bits.size());
        Pushed p;
        p.out.resize(no + 1);
        if (want_audio) p.audio.resize(na + 1);
        size_t o = 0, a = 0;
        if (rr_fsk_tx_push(h_.h, bits.data(), bits.size(), reinterpret_cast<rr_c32*>(p.out.data()), no,
                           want_audio ? p.audio.data() : nullptr, want_audio ? na : 0, &o, &a) != 0)
            throw Error(rr_last_error());
        p.out.resize(std::min(o, no));
        if (want_audio) p.audio.resize(std::min(a, na));
        return p;
    }
    // device pointers; asynchronous on hip_stream -> (n_out, n_audio), there when the call returns
    std::pair<size_t, size_t> push_dev(const void* d_bits, size_t n_bits, void* d_out, size_t out_cap, void* d_audio = nullptr,
                                       size_t audio_cap = 0, void* hip_stream = nullptr) {
        size_t o = 0, a = 0;
        if (rr_fsk_tx_push_dev(h_.h, d_bits, n_bits, d_out, out_cap, d_audio, audio_cap, &o, &a, hip_stream) != 0) throw Error(rr_last_error());
        return {o, a};
    }
    size_t audio_tile() const { size_t a = 0, o = 0, c = 0; if (rr_fsk_tx_dims(h_.h, &a, &o, &c) != 0) throw Error(rr_last_error()); return a; }
    size_t out_tile() const { size_t a = 0, o = 0, c = 0; if (rr_fsk_tx_dims(h_.h, &a, &o, &c) != 0) throw Error(rr_last_error()); return o; }
    size_t scan_chunk_tiles() const { size_t a = 0, o = 0, c = 0; if (rr_fsk_tx_dims(h_.h, &a, &o, &c) != 0) throw Error(rr_last_error()); return c; }
};

// ---- FskTxMulti: FskTx x nstreams of one parameter set behind one handle, the counts of a push read on the device ------------------
// (rr_fsk_tx_multi_create / _bound / _push / _push_dev / _counts / _counts_dev / _positions / _dims).  push() takes one row of
// line bits per stream, of which stream c holds counts[c], and returns what each stream made.
class FskTxMulti {
    detail::Handle h_;
    size_t nstreams_;
public:
    struct Pushed {
        std::vector<std::vector<Complex>> out;    // per stream
        std::vector<std::vector<float>> audio;    // AFSK mode with audio asked for
    };
    FskTxMulti(size_t nstreams, int mode, size_t interp1, size_t deci1, float lo, float hi, double k1, float gain, size_t interp2 = 1,
               size_t deci2 = 1, double k2 = 0.0)
        : h_(rr_fsk_tx_multi_create(nstreams, mode, interp1, deci1, lo, hi, detail::f64_bits(k1), gain, interp2, deci2,
                                    detail::f64_bits(k2))),
          nstreams_(nstreams) {}
    rr_block* handle() const { return h_.h; }
    size_t nstreams() const { return nstreams_; }
    // (audio_cap, out_cap): the most one stream makes from n_cap bits
    std::pair<size_t, size_t> bound(size_t n_cap) const {
        size_t a = 0, o = 0;
        if (rr_fsk_tx_multi_bound(h_.h, n_cap, &a, &o) != 0) throw Error(rr_last_error());
        return {a, o};
    }
    // rows: nstreams rows of one length n_cap; counts: empty (n_cap each) or one per stream
    Pushed push(const std::vector<std::vector<unsigned char>>& rows, const std::vector<size_t>& counts = {}, bool want_audio = false) {
        if (rows.size() != nstreams_) throw Error("FskTxMulti: one row per stream");
        if (!counts.empty() && counts.size() != nstreams_) throw Error("FskTxMulti: one count per stream");
        const size_t n = rows[0].size();
        std::vector<unsigned char> bits(nstreams_ * n + 1);
        for (size_t c = 0; c < nstreams_; c++) {
            if (rows[c].size() != n) throw Error("FskTxMulti: rows of one length");
            std::copy(rows[c].begin(), rows[c].end(), bits.begin() + (long)(c * n));
        }
        const auto [ac, oc] = bound(n);
        std::vector<Complex> out(nstreams_ * oc + 1);
        std::vector<float> audio(want_audio ? nstreams_ * ac + 1 : 0);
        std::vector<size_t> no(nstreams_), na(nstreams_);
        if (rr_fsk_tx_multi_push(h_.h, bits.data(), n, n, counts.empty() ? nullptr : counts.data(), reinterpret_cast<rr_c32*>(out.data()),
                                 oc, want_audio ? audio.data() : nullptr, want_audio ? ac : 0, no.data(), na.data()) != 0)
            throw Error(rr_last_error());
        Pushed p;
        p.out.resize(nstreams_);
        if (want_audio) p.audio.resize(nstreams_);
        for (size_t c = 0; c < nstreams_; c++) {
            p.out[c].assign(out.begin() + (long)(c * oc), out.begin() + (long)(c * oc + std::min(no[c], oc)));
            if (want_audio) p.audio[c].assign(audio.begin() + (long)(c * ac), audio.begin() + (long)(c * ac + std::min(na[c], ac)));
        }
        return p;
    }
    // device pointers; d_counts: unsigned long long[nstreams] on the device or nullptr; asynchronous on hip_stream
    void push_dev(const void* d_bits, size_t bits_stride, size_t n_cap, const void* d_counts, void* d_out, size_t out_stride,
                  void* d_audio = nullptr, size_t audio_stride = 0, void* hip_stream = nullptr) {
        if (rr_fsk_tx_multi_push_dev(h_.h, d_bits, bits_stride, n_cap, d_counts, d_out, out_stride, d_audio, audio_stride, hip_stream) != 0)
            throw Error(rr_last_error());
    }
    // (n_audio, n_out) of each stream in the most recent push; waits for it
    std::vector<std::pair<size_t, size_t>> counts() {
        std::vector<size_t> a(nstreams_), o(nstreams_);
        size_t total = 0;
        if (rr_fsk_tx_multi_counts(h_.h, a.data(), o.data(), nstreams_, &total) != 0) throw Error(rr_last_error());
        std::vector<std::pair<size_t, size_t>> k(std::min(total, nstreams_));
        for (size_t c = 0; c < k.size(); c++) k[c] = {a[c], o[c]};
        return k;
    }
    const void* counts_dev() { return rr_fsk_tx_multi_counts_dev(h_.h); }
    // bits taken, audio samples and outputs made by stream c so far; waits
    struct Position { unsigned long long bits, audio, out; };
    std::vector<Position> positions() {
        std::vector<unsigned long long> b(nstreams_), a(nstreams_), o(nstreams_);
        size_t total = 0;
        if (rr_fsk_tx_multi_positions(h_.h, b.data(), a.data(), o.data(), nstreams_, &total) != 0) throw Error(rr_last_error());
        std::vector<Position> p(std::min(total, nstreams_));
        for (size_t c = 0; c < p.size(); c++) p[c] = {b[c], a[c], o[c]};
        return p;
    }
    size_t audio_tile() const { size_t a = 0, o = 0, c = 0; if (rr_fsk_tx_multi_dims(h_.h, &a, &o, &c) != 0) throw Error(rr_last_error()); return a; }
    size_t out_tile() const { size_t a = 0, o = 0, c = 0; if (rr_fsk_tx_multi_dims(h_.h, &a, &o, &c) != 0) throw Error(rr_last_error()); return o; }
    size_t scan_chunk_tiles() const { size_t a = 0, o = 0, c = 0; if (rr_fsk_tx_multi_dims(h_.h, &a, &o, &c) != 0) throw Error(rr_last_error()); return c; }
};

class Vco : public SyncBlock<Float, Complex> {
public:
    using SyncBlock<Float, Complex>::SyncBlock;
    static std::pair<std::unique_ptr<Vco>, ReadStream<Complex>> new_(ReadStream<Float> src, double k) {
        auto [w, r] = new_stream<Complex>();
        return {std::make_unique<Vco>(rr_vco_create(detail::f64_bits(k)), std::move(src), std::move(w)), std::move(r)};
    }
};

// ComplexToMag2 (src/complex_to_mag2.rs:8-21) and SinglePoleIirFilter<Float|Complex> (src/single_pole_iir_filter.rs:11-93): sync
// blocks.  SinglePoleIirFilter::new_ returns an empty optional for an alpha outside 0..=1 (NaN included), the reference's None.
class ComplexToMag2 : public SyncBlock<Complex, Float> {
public:
    using SyncBlock<Complex, Float>::SyncBlock;
    static std::pair<std::unique_ptr<ComplexToMag2>, ReadStream<Float>> new_(ReadStream<Complex> src) {
        auto [w, r] = new_stream<Float>();
        return {std::make_unique<ComplexToMag2>(rr_complex_to_mag2_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
// The first Map of examples/airspy_am_decode.rs ("AirSPY to Complex"): u32 words (i16 I low, i16 Q high) -> Complex(i / 1000, q / 1000)
class AirspyDecode : public SyncBlock<uint32_t, Complex> {
public:
    using SyncBlock<uint32_t, Complex>::SyncBlock;
    static std::pair<std::unique_ptr<AirspyDecode>, ReadStream<Complex>> new_(ReadStream<uint32_t> src) {
        auto [w, r] = new_stream<Complex>();
        return {std::make_unique<AirspyDecode>(rr_airspy_decode_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
template <class T> class SinglePoleIirFilter : public SyncBlock<T, T> {
public:
    using SyncBlock<T, T>::SyncBlock;
    static std::optional<std::pair<std::unique_ptr<SinglePoleIirFilter<T>>, ReadStream<T>>> new_(ReadStream<T> src, Float alpha) {
        if (!(alpha >= 0.0f && alpha <= 1.0f)) return std::nullopt;                // :38-41
        auto [w, r] = new_stream<T>();
        return std::make_pair(std::make_unique<SinglePoleIirFilter<T>>(rr_single_pole_iir_create(alpha, sizeof(T)), std::move(src), std::move(w)),
                              std::move(r));
    }
};

// ---- the bit-level sync blocks behind a symbol clock (examples/ax25-9600-rx.rs:195-204, examples/il2p-1200-rx.rs:118-126) -----
// BinarySlicer (src/binary_slicer.rs:8-20), NrziDecode (src/nrzi.rs:25-42), Descrambler (src/descrambler.rs:50-93) are sync
// blocks; CorrelateAccessCodeTag (src/correlate_access_code.rs:58-119) is a sync_tag block: the data passes through and every
// match adds Tag(pos, tag, U64(diffs)) BEHIND the input's own tags at that position, as process_sync_tags orders them.
// BitDecoder is the fusion of all of them (rr_bit_decoder_create).  A constructor the C ABI refuses throws its message.
class BinarySlicer : public SyncBlock<Float, uint8_t> {
public:
    using SyncBlock<Float, uint8_t>::SyncBlock;
    static std::pair<std::unique_ptr<BinarySlicer>, ReadStream<uint8_t>> new_(ReadStream<Float> src) {
        auto [w, r] = new_stream<uint8_t>();
        return {std::make_unique<BinarySlicer>(rr_binary_slicer_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
class NrziDecode : public SyncBlock<uint8_t, uint8_t> {
public:
    using SyncBlock<uint8_t, uint8_t>::SyncBlock;
    static std::pair<std::unique_ptr<NrziDecode>, ReadStream<uint8_t>> new_(ReadStream<uint8_t> src) {
        auto [w, r] = new_stream<uint8_t>();
        return {std::make_unique<NrziDecode>(rr_nrzi_decode_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
// NrziEncode (src/nrzi.rs:52-69) and Scrambler (src/descrambler.rs:95-123): the transmit side's sync blocks, u8 in, u8 out
class NrziEncode : public SyncBlock<uint8_t, uint8_t> {
public:
    using SyncBlock<uint8_t, uint8_t>::SyncBlock;
    static std::pair<std::unique_ptr<NrziEncode>, ReadStream<uint8_t>> new_(ReadStream<uint8_t> src) {
        auto [w, r] = new_stream<uint8_t>();
        return {std::make_unique<NrziEncode>(rr_nrzi_encode_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
class Scrambler : public SyncBlock<uint8_t, uint8_t> {
public:
    using SyncBlock<uint8_t, uint8_t>::SyncBlock;
    static std::pair<std::unique_ptr<Scrambler>, ReadStream<uint8_t>> g3ruh(ReadStream<uint8_t> src) {         // :106-118
        auto [w, r] = new_stream<uint8_t>();
        return {std::make_unique<Scrambler>(rr_scrambler_g3ruh_create(), std::move(src), std::move(w)), std::move(r)};
    }
};
class Descrambler : public SyncBlock<uint8_t, uint8_t> {
public:
    using SyncBlock<uint8_t, uint8_t>::SyncBlock;
    static std::pair<std::unique_ptr<Descrambler>, ReadStream<uint8_t>> new_(ReadStream<uint8_t> src, uint64_t mask, uint64_t seed,
                                                                              unsigned len) {
        auto [w, r] = new_stream<uint8_t>();
        return {std::make_unique<Descrambler>(rr_descrambler_create(mask, seed, len), std::move(src), std::move(w)), std::move(r)};
    }
    static std::pair<std::unique_ptr<Descrambler>, ReadStream<uint8_t>> g3ruh(ReadStream<uint8_t> src) {      // :78-88
        return new_(std::move(src), 0x21, 0, 16);
    }
};
namespace detail {
// an access code as the C ABI takes it: bit k of the word = code[k], code[0] the oldest bit; the length goes along unclipped
inline unsigned long long pack_code(const std::vector<uint8_t>& code) {
    unsigned long long w = 0;
    for (size_t k = 0; k < code.size(); k++) {
        if (code[k] > 1) throw Error("access code bits must be 0 or 1");
        if (k < 64) w |= (unsigned long long)code[k] << k;
    }
    return w;
}
// a sync block whose handle has a correlator stage: the forwarded input tags, then the handle's own (rr_bit_tags)
template <class In> class SyncTagBlock : public SyncBlock<In, uint8_t> {
    std::string tag_;
    bool corr_;
    std::vector<size_t> pos_;
    std::vector<unsigned char> diffs_;
public:
    SyncTagBlock(rr_block* h, ReadStream<In> src, WriteStream<uint8_t> dst, std::string tag, bool corr)
        : SyncBlock<In, uint8_t>(h, std::move(src), std::move(dst)), tag_(std::move(tag)), corr_(corr) {}
    BlockRet work() override {
        auto [input, tags] = this->src_.read_buf();
        auto out = this->dst_.write_buf();
        auto w = detail::work(this->h_.h, input, out);
        std::vector<Tag> keep;
        for (auto& t : tags) if (t.pos() < w.produced) keep.push_back(t);
        if (corr_ && w.produced) {
            size_t total = 0;
            if (rr_bit_tags(this->h_.h, nullptr, nullptr, 0, &total) != 0) throw Error(rr_last_error());
            pos_.resize(total); diffs_.resize(total);
            if (total && rr_bit_tags(this->h_.h, pos_.data(), diffs_.data(), total, &total) != 0) throw Error(rr_last_error());
            for (size_t j = 0; j < total; j++) keep.emplace_back(pos_[j], tag_, (uint64_t)diffs_[j]);
            std::stable_sort(keep.begin(), keep.end(), [](const Tag& a, const Tag& b) { return a.pos() < b.pos(); });
        }
        input.consume(w.consumed);
        out.produce(w.produced, keep);
        return w.st == RR_WAIT_DST ? BlockRet::wait(this->dst_.wait_handle(), w.need) : BlockRet::wait(this->src_.wait_handle(), w.need);
    }
};
}  // namespace detail
class CorrelateAccessCodeTag : public detail::SyncTagBlock<uint8_t> {
public:
    using detail::SyncTagBlock<uint8_t>::SyncTagBlock;
    static std::pair<std::unique_ptr<CorrelateAccessCodeTag>, ReadStream<uint8_t>> new_(ReadStream<uint8_t> src, const std::vector<uint8_t>& code,
                                                                                         std::string tag, size_t allowed_diffs) {
        auto [w, r] = new_stream<uint8_t>();
        rr_block* h = rr_correlate_access_code_tag_create(detail::pack_code(code), (unsigned)code.size(), allowed_diffs);
        return {std::make_unique<CorrelateAccessCodeTag>(h, std::move(src), std::move(w), std::move(tag), true), std::move(r)};
    }
};
// flags: RR_BITS_INVERT | RR_BITS_NRZI | RR_BITS_DESCRAMBLE; mask, seed, len are read only with RR_BITS_DESCRAMBLE; an empty code:
// no correlator and no tags of its own
class BitDecoder : public detail::SyncTagBlock<Float> {
public:
    using detail::SyncTagBlock<Float>::SyncTagBlock;
    static std::pair<std::unique_ptr<BitDecoder>, ReadStream<uint8_t>> new_(ReadStream<Float> src, int flags, uint64_t mask, uint64_t seed,
                                                                             unsigned len, const std::vector<uint8_t>& code, std::string tag,
                                                                             size_t allowed_diffs) {
        auto [w, r] = new_stream<uint8_t>();
        rr_block* h = rr_bit_decoder_create(flags, mask, seed, len, detail::pack_code(code), (unsigned)code.size(), allowed_diffs);
        return {std::make_unique<BitDecoder>(h, std::move(src), std::move(w), std::move(tag), !code.empty()), std::move(r)};
    }
};

// ---- graph-level fusions (one block, one kernel; whole-stream output = the reference blocks in sequence) ------------------
// Tags: what the reference blocks in sequence would deliver (rr_block_tag_rule) — a chain holding a RationalResampler or a
// QuadratureDemod drops them, FirFilter -> FftFilter and Hilbert -> FirFilter forward them.
template <class In, class Out> class Fused : public Block {
    detail::Handle h_;
    ReadStream<In> src_;
    WriteStream<Out> dst_;
    detail::TagForwarder fwd_;
public:
    Fused(rr_block* h, ReadStream<In> src, WriteStream<Out> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)), fwd_(h_.h) {}
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        const std::vector<Tag> emit = fwd_.step(tags, w.consumed, w.produced);
        input.consume(w.consumed);
        out.produce(w.produced, emit);
        if (w.st == RR_AGAIN) return BlockRet::again();
        return w.st == RR_WAIT_DST ? BlockRet::wait(dst_.wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
    template <class MakeHandle> static std::pair<std::unique_ptr<Fused>, ReadStream<Out>> make(ReadStream<In> src, MakeHandle&& mk) {
        auto [w, r] = new_stream<Out>();
        return {std::make_unique<Fused>(mk(), std::move(src), std::move(w)), std::move(r)};
    }
};
inline const rr_c32* c32(const std::vector<Complex>& v) { return reinterpret_cast<const rr_c32*>(v.data()); }
// FftFilter -> RationalResampler -> QuadratureDemod (examples/rtl_fm.rs:381-419)
inline auto FmChain(ReadStream<Complex> src, const std::vector<Complex>& taps, size_t interp, size_t deci, Float gain, bool exact_atan2 = true) {
    return Fused<Complex, Float>::make(std::move(src), [&] { return rr_fm_chain_create(c32(taps), taps.size(), interp, deci, gain, exact_atan2 ? RR_ATAN2_EXACT : RR_ATAN2_FAST); });
}
// FftFilter -> RationalResampler fused, Complex out (rr_channelizer_create with one channel; examples/rtl_downsampled.rs:37-52)
inline auto FftFilterResampler(ReadStream<Complex> src, const std::vector<Complex>& taps, size_t interp, size_t deci) {
    return Fused<Complex, Complex>::make(std::move(src), [&] { return rr_channelizer_create(c32(taps), 1, taps.size(), interp, deci); });
}
// FirFilter -> FftFilter as one convolution (the north star's pair)
inline auto FirFftFilter(ReadStream<Complex> src, const std::vector<Complex>& fir_taps, const std::vector<Complex>& fft_taps) {
    return Fused<Complex, Complex>::make(std::move(src), [&] { return rr_fir_fftfilter_create(c32(fir_taps), fir_taps.size(), c32(fft_taps), fft_taps.size()); });
}
// FirFilter -> FftFilter -> RationalResampler -> QuadratureDemod (BASELINE's metric chain)
inline auto FirFmChain(ReadStream<Complex> src, const std::vector<Complex>& fir_taps, const std::vector<Complex>& fft_taps, size_t interp,
                       size_t deci, Float gain, bool exact_atan2 = true) {
    return Fused<Complex, Float>::make(std::move(src), [&] {
        return rr_fir_fm_chain_create(c32(fir_taps), fir_taps.size(), c32(fft_taps), fft_taps.size(), interp, deci, gain,
                                      exact_atan2 ? RR_ATAN2_EXACT : RR_ATAN2_FAST);
    });
}
// Hilbert -> FirFilter(deci)[.translate(samp_rate, freq)] (BASELINE configs[4]; hilbert.rs:38-129 + fir.rs:303-551)
inline auto HilbertFir(ReadStream<Float> src, size_t hilbert_ntaps, const window::WindowType& w, const std::vector<Complex>& taps,
                       size_t deci, bool translate = false, Float samp_rate = 0, Float freq = 0) {
    return Fused<Float, Complex>::make(std::move(src), [&] {
        return rr_hilbert_fir_create(hilbert_ntaps, w.kind, w.parm, c32(taps), taps.size(), deci, translate, samp_rate, freq);
    });
}
// FftFilterFloat -> RationalResampler -> MultiplyConst (examples/rtl_fm.rs:398-418)
inline auto AudioChain(ReadStream<Float> src, const std::vector<Float>& taps, size_t interp, size_t deci, Float scale) {
    return Fused<Float, Float>::make(std::move(src), [&] { return rr_audio_chain_create(taps.data(), taps.size(), interp, deci, scale); });
}
// RationalResampler(interp, deci) -> Vco(k) (examples/fm_tx.rs:84-91): the resampler's window protocol and eof, tags dropped
struct FmTx {
    static auto new_(ReadStream<Float> src, size_t interp, size_t deci, double k) {
        return Fused<Float, Complex>::make(std::move(src), [&] { return rr_fm_tx_create(interp, deci, detail::f64_bits(k)); });
    }
};

// Delay::new(src, delay) (src/delay.rs): `delay` default elements, then the input; tags move `delay` outputs on (RR_TAGS_SHIFT).
// T of 1, 4 or 8 bytes.  set_delay is not offered.
template <class T> struct Delay {
    static auto new_(ReadStream<T> src, size_t delay) {
        return Fused<T, T>::make(std::move(src), [&] { return rr_delay_create(delay, sizeof(T)); });
    }
};

// The burst path of examples/burst_saver.rs:111-123 as one block (rr_burst_detector_create): Tee, ComplexToMag2,
// SinglePoleIirFilter(alpha) and BurstTagger(threshold, tag).  The DATA stream passes through unchanged, as BurstTagger does
// (src/burst_tagger.rs:68-85); the filtered power stays in a private scratch, and where it crosses the threshold the output
// gets Tag(pos, tag, Bool(cur)) next to the input's own tags: process_sync_tags in one place.  Feeds StreamToPdu directly.
// Throws for an alpha outside 0..=1 (where SinglePoleIirFilter::new returns None in the reference's wiring).
class BurstDetector : public Block {
    detail::Handle h_;
    ReadStream<Complex> src_;
    WriteStream<Complex> dst_;
    std::string tag_;
    std::vector<Float> env_;
    std::vector<size_t> pos_;
    std::vector<unsigned char> val_;
public:
    BurstDetector(rr_block* h, ReadStream<Complex> src, WriteStream<Complex> dst, std::string tag)
        : h_(h), src_(std::move(src)), dst_(std::move(dst)), tag_(std::move(tag)) {}
    static std::pair<std::unique_ptr<BurstDetector>, ReadStream<Complex>> new_(ReadStream<Complex> src, Float alpha, Float threshold,
                                                                               std::string tag) {
        auto [w, r] = new_stream<Complex>();
        return {std::make_unique<BurstDetector>(rr_burst_detector_create(alpha, threshold), std::move(src), std::move(w), std::move(tag)),
                std::move(r)};
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        if (input.device() || out.device()) throw Error("BurstDetector: host streams only (the data stream is copied on the host)");
        env_.resize(std::max<size_t>(out.len(), 1));
        auto w = detail::work(h_.h, input.slice(), input.len(), env_.data(), out.len());     // n = min(in, out) samples
        std::vector<Tag> keep;
        for (auto& t : tags) if (t.pos() < w.produced) keep.push_back(t);
        if (w.produced) {
            out.fill_from_slice(input.slice(), w.produced);
            size_t total = 0;
            if (rr_burst_edges(h_.h, nullptr, nullptr, 0, &total) != 0) throw Error(rr_last_error());
            pos_.resize(total); val_.resize(total);
            if (total && rr_burst_edges(h_.h, pos_.data(), val_.data(), total, &total) != 0) throw Error(rr_last_error());
            for (size_t j = 0; j < total; j++) keep.emplace_back(pos_[j], tag_, val_[j] != 0);
            std::stable_sort(keep.begin(), keep.end(), [](const Tag& a, const Tag& b) { return a.pos() < b.pos(); });
        }
        input.consume(w.consumed);
        out.produce(w.produced, keep);
        return w.st == RR_WAIT_DST ? BlockRet::wait(dst_.wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
};

// The N-station FM receiver down to audio (rr_fm_receiver_create): Tee (src/tee.rs:10-24) + N x the six blocks of
// examples/rtl_fm.rs:381-419 on ONE input, N audio streams.  The C ABI takes the N output windows as one buffer of N x out_cap
// elements, so the block stages them in `scratch_` and copies each channel into its own (host) stream; the resamplers drop tags.
class FmReceiver : public Block {
    detail::Handle h_;
    ReadStream<Complex> src_;
    std::vector<WriteStream<Float>> dsts_;
    std::vector<Float> scratch_;
public:
    FmReceiver(rr_block* h, ReadStream<Complex> src, std::vector<WriteStream<Float>> dsts)
        : h_(h), src_(std::move(src)), dsts_(std::move(dsts)) {}
    // rf_taps[c] = channel c's RF filter (all of one length); audio_taps is shared by the channels, as in rtl_fm
    static std::pair<std::unique_ptr<FmReceiver>, std::vector<ReadStream<Float>>> new_(
        ReadStream<Complex> src, const std::vector<std::vector<Complex>>& rf_taps, size_t rf_interp, size_t rf_deci, Float gain,
        const std::vector<Float>& audio_taps, size_t audio_interp, size_t audio_deci, Float scale, bool exact_atan2 = true) {
        const size_t nchan = rf_taps.size(), ntaps = nchan ? rf_taps[0].size() : 0;
        std::vector<Complex> flat;
        for (auto& t : rf_taps) {
            if (t.size() != ntaps) throw Error("FmReceiver: all channels need the same number of taps");
            flat.insert(flat.end(), t.begin(), t.end());
        }
        rr_block* h = rr_fm_receiver_create(c32(flat), nchan, ntaps, rf_interp, rf_deci, gain, exact_atan2 ? RR_ATAN2_EXACT : RR_ATAN2_FAST,
                                            audio_taps.data(), audio_taps.size(), audio_interp, audio_deci, scale);
        std::vector<WriteStream<Float>> ws;
        std::vector<ReadStream<Float>> rs;
        for (size_t c = 0; c < nchan; c++) {
            auto [w, r] = new_stream<Float>();
            ws.push_back(std::move(w));
            rs.push_back(std::move(r));
        }
        return {std::make_unique<FmReceiver>(h, std::move(src), std::move(ws)), std::move(rs)};
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        (void)tags;
        std::vector<BufferWriter<Float>> outs;
        size_t cap = ~(size_t)0;
        for (auto& d : dsts_) {
            outs.push_back(d.write_buf());
            if (outs.back().device() || input.device()) throw Error("FmReceiver: host streams only (N output windows are one buffer in the C ABI)");
            cap = std::min(cap, outs.back().len());
        }
        scratch_.resize(dsts_.size() * std::max<size_t>(cap, 1));
        auto w = detail::work(h_.h, input.slice(), input.len(), scratch_.data(), cap);
        for (size_t c = 0; c < outs.size(); c++) {
            outs[c].fill_from_slice(scratch_.data() + c * cap, w.produced);
            outs[c].produce(w.produced, {});
        }
        input.consume(w.consumed);
        if (w.st == RR_AGAIN) return BlockRet::again();
        return w.st == RR_WAIT_DST ? BlockRet::wait(dsts_[0].wait_handle(), w.need) : BlockRet::wait(src_.wait_handle(), w.need);
    }
};

// ---- Hilbert (src/hilbert.rs) ----------------------------------------------------------------------------------------------
class Hilbert : public Block {
    detail::Handle h_;
    ReadStream<Float> src_;
    WriteStream<Complex> dst_;
public:
    Hilbert(rr_block* h, ReadStream<Float> src, WriteStream<Complex> dst) : h_(h), src_(std::move(src)), dst_(std::move(dst)) {}
    // asserts odd ntaps > 1 in the reference (:44-47); here: throws Error
    static std::pair<std::unique_ptr<Hilbert>, ReadStream<Complex>> new_(ReadStream<Float> src, size_t ntaps, const window::WindowType& w) {
        auto [ws, r] = new_stream<Complex>();
        rr_block* h = rr_hilbert_create(ntaps, w.kind, w.parm);
        return {std::make_unique<Hilbert>(h, std::move(src), std::move(ws)), std::move(r)};
    }
    const char* block_name() const override { return rr_block_name(h_.h); }
    bool eof() override { return rr_block_eof(h_.h, src_.eof()) != 0; }
    BlockRet work() override {                    // :72-128
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        auto w = detail::work(h_.h, input, out);
        if (w.st == RR_WAIT_SRC) { out.produce(0, {}); return BlockRet::wait(src_.wait_handle(), w.need); }
        if (w.st == RR_WAIT_DST) { out.produce(0, {}); return BlockRet::wait(dst_.wait_handle(), w.need); }
        std::vector<Tag> keep;                    // :119-123
        for (auto& t : tags) if (t.pos() < w.produced) keep.push_back(t);
        out.produce(w.produced, keep);
        input.consume(w.consumed);
        return BlockRet::again();
    }
};

// ---- harness blocks (restated from the reference; host-side plumbing only) ----------------------------------------------------
struct Repeat {                                   // src/lib.rs Repeat
    uint64_t count; bool infinite;
    static Repeat finite(uint64_t n) { return {n, false}; }
    static Repeat infinite_() { return {0, true}; }
};

template <class T> class VectorSource : public Block {   // src/vector_source.rs:97-146
    WriteStream<T> dst_;
    std::vector<T> data_;
    Repeat repeat_;
    uint64_t repeat_count_ = 0;
    size_t pos_ = 0;
public:
    VectorSource(WriteStream<T> dst, std::vector<T> d, Repeat r) : dst_(std::move(dst)), data_(std::move(d)), repeat_(r) {}
    static std::pair<std::unique_ptr<VectorSource<T>>, ReadStream<T>> new_(std::vector<T> data, Repeat r = Repeat::finite(1)) {
        auto [w, rd] = new_stream<T>();
        return {std::make_unique<VectorSource<T>>(std::move(w), std::move(data), r), std::move(rd)};
    }
    const char* block_name() const override { return "VectorSource"; }
    bool eof() override { return !repeat_.infinite && repeat_count_ >= repeat_.count; }
    BlockRet work() override {
        if (eof() || data_.empty()) return BlockRet::eof();
        auto out = dst_.write_buf();
        const size_t n = std::min(out.len(), data_.size() - pos_);
        if (n == 0) { out.produce(0, {}); return BlockRet::wait(dst_.wait_handle(), 1); }
        std::vector<Tag> tags;
        if (pos_ == 0) {
            tags.emplace_back(0, "VectorSource::start", true);
            tags.emplace_back(0, "VectorSource::repeat", (uint64_t)repeat_count_);
            if (repeat_count_ == 0) tags.emplace_back(0, "VectorSource::first", true);
        }
        out.fill_from_slice(data_.data() + pos_, n);
        out.produce(n, tags);
        pos_ += n;
        if (pos_ == data_.size()) { pos_ = 0; repeat_count_++; }
        return eof() ? BlockRet::eof() : BlockRet::again();
    }
};

// FileSource<T> (src/file_source.rs:43-153): raw little-endian samples (`.c32` = interleaved f32 re, im; `.u8`
// RTL-SDR bytes, ...) from disk into a stream of any placement; a partial trailing sample is dropped at EOF
// (and on repeat), as the reference does.
template <class T> class FileSource : public Block {
    WriteStream<T> dst_;
    std::string filename_;
    FILE* f_ = nullptr;
    Repeat repeat_;
    uint64_t count_ = 0;                        // Repeat::again() counter (src/lib.rs:477-490)
    std::vector<uint8_t> buf_;                  // bytes of an incomplete sample + not yet emitted samples
    std::vector<uint8_t> rd_;
    bool again() { count_++; return repeat_.infinite || count_ < repeat_.count; }
public:
    FileSource(WriteStream<T> dst, std::string filename, Repeat r) : dst_(std::move(dst)), filename_(std::move(filename)), repeat_(r) {
        f_ = std::fopen(filename_.c_str(), "rb");
        if (!f_) throw Error("FileSource: cannot open " + filename_);       // Error::file_io (:64-66)
    }
    ~FileSource() override { if (f_) std::fclose(f_); }
    static std::pair<std::unique_ptr<FileSource<T>>, ReadStream<T>> new_(const std::string& filename, Repeat r = Repeat::finite(1)) {
        auto [w, rd] = new_stream<T>();
        return {std::make_unique<FileSource<T>>(std::move(w), filename, r), std::move(rd)};
    }
    const char* block_name() const override { return "FileSource"; }
    bool eof() override { return false; }
    BlockRet work() override {                  // :89-152
        auto o = dst_.write_buf();
        constexpr size_t ss = sizeof(T);
        size_t have = buf_.size() / ss;
        const size_t want = o.len();
        if (want == 0) { o.produce(0, {}); return BlockRet::wait(dst_.wait_handle(), 1); }
        if (have < want) {
            rd_.resize((want - have) * ss);
            const size_t n = std::fread(rd_.data(), 1, rd_.size(), f_);
            if (n == 0) {
                o.produce(0, {});
                if (again()) {
                    buf_.clear();
                    std::fseek(f_, 0, SEEK_SET);
                    return BlockRet::again();
                }
                return BlockRet::eof();
            }
            if (buf_.empty() && n % ss == 0) {  // fast path: whole samples only (:120-128)
                o.fill_from_slice(reinterpret_cast<const T*>(rd_.data()), n / ss);
                o.produce(n / ss, {});
                return BlockRet::again();
            }
            buf_.insert(buf_.end(), rd_.begin(), rd_.begin() + (std::ptrdiff_t)n);
        }
        have = buf_.size() / ss;
        if (have == 0) { o.produce(0, {}); return BlockRet{BlockRet::Pending, nullptr, 0}; }
        const size_t nemit = std::min(have, want);
        std::vector<T> tmp(nemit);
        std::memcpy(tmp.data(), buf_.data(), nemit * ss);
        buf_.erase(buf_.begin(), buf_.begin() + (std::ptrdiff_t)(nemit * ss));
        o.fill_from_slice(tmp.data(), nemit);
        o.produce(nemit, {});
        return BlockRet::again();
    }
};

template <class T> class VectorSink : public Block {     // src/vector_sink.rs:113-137
    ReadStream<T> src_;
    std::shared_ptr<std::vector<T>> data_ = std::make_shared<std::vector<T>>();
    std::shared_ptr<std::vector<Tag>> tags_ = std::make_shared<std::vector<Tag>>();
public:
    explicit VectorSink(ReadStream<T> src) : src_(std::move(src)) {}
    std::shared_ptr<std::vector<T>> hook() const { return data_; }           // vector_sink.rs:103-111
    std::shared_ptr<std::vector<Tag>> tag_hook() const { return tags_; }
    const char* block_name() const override { return "VectorSink"; }
    bool eof() override { return src_.eof(); }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        const size_t n = input.len();
        for (auto& t : tags) tags_->emplace_back(t.pos() + data_->size(), t.key(), t.val());
        const size_t at = data_->size();
        data_->resize(at + n);
        input.copy_to(data_->data() + at, n);
        input.consume(n);
        return BlockRet::wait(src_.wait_handle(), 1);
    }
};

template <class T> class NullSink : public Block {       // src/null_sink.rs:15-25
    ReadStream<T> src_;
public:
    explicit NullSink(ReadStream<T> src) : src_(std::move(src)) {}
    const char* block_name() const override { return "NullSink"; }
    bool eof() override { return src_.eof(); }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        (void)tags;
        input.consume(input.len());
        return BlockRet::wait(src_.wait_handle(), 1);
    }
};

// Moves samples (and tags) between streams of any placement: the explicit upload / download step of a
// graph that mixes CPU blocks and device-resident GPU chains.  No reference counterpart.
template <class T> class MemCopy : public Block {
    ReadStream<T> src_;
    WriteStream<T> dst_;
    std::vector<T> bounce_;
public:
    MemCopy(ReadStream<T> src, WriteStream<T> dst) : src_(std::move(src)), dst_(std::move(dst)) {}
    static std::pair<std::unique_ptr<MemCopy<T>>, ReadStream<T>> new_(ReadStream<T> src, Memory to) {
        auto [w, r] = new_stream<T>(default_stream_size(), to);
        return {std::make_unique<MemCopy<T>>(std::move(src), std::move(w)), std::move(r)};
    }
    const char* block_name() const override { return "MemCopy"; }
    bool eof() override { return src_.eof(); }
    BlockRet work() override {
        auto [input, tags] = src_.read_buf();
        auto out = dst_.write_buf();
        const size_t n = std::min(input.len(), out.len());
        if (n == 0) {
            out.produce(0, {});
            return input.len() == 0 ? BlockRet::wait(src_.wait_handle(), 1) : BlockRet::wait(dst_.wait_handle(), 1);
        }
        std::vector<Tag> keep;
        for (auto& t : tags) if (t.pos() < n) keep.push_back(t);
        if (!input.device()) out.fill_from_slice(input.slice(), n);
        else if (!out.device()) input.copy_to(out.slice(), n);
        else out.fill_from_device(input, n);                              // HBM ring to HBM ring: device-to-device
        input.consume(n);
        out.produce(n, keep);
        return BlockRet::again();
    }
};

// Tee (src/tee.rs:10-24): every input sample and tag goes to both outputs.
template <class T> class Tee : public Block {
    ReadStream<T> src_;
    WriteStream<T> dst1_, dst2_;
    std::vector<T> bounce_;
public:
    Tee(ReadStream<T> src, WriteStream<T> d1, WriteStream<T> d2) : src_(std::move(src)), dst1_(std::move(d1)), dst2_(std::move(d2)) {}
    static std::tuple<std::unique_ptr<Tee<T>>, ReadStream<T>, ReadStream<T>> new_(ReadStream<T> src) {
        auto [w1, r1] = new_stream<T>();
        auto [w2, r2] = new_stream<T>();
        return {std::make_unique<Tee<T>>(std::move(src), std::move(w1), std::move(w2)), std::move(r1), std::move(r2)};
    }
    const char* block_name() const override { return "Tee"; }
    bool eof() override { return src_.eof(); }
    BlockRet work() override {                    // the `sync` macro loop: min over the input and both outputs
        auto [input, tags] = src_.read_buf();
        auto o1 = dst1_.write_buf();
        auto o2 = dst2_.write_buf();
        const size_t n = std::min(input.len(), std::min(o1.len(), o2.len()));
        if (n == 0) {
            o1.produce(0, {}); o2.produce(0, {});
            if (input.len() == 0) return BlockRet::wait(src_.wait_handle(), 1);
            return BlockRet::wait(o1.len() == 0 ? dst1_.wait_handle() : dst2_.wait_handle(), 1);
        }
        std::vector<Tag> keep;
        for (auto& t : tags) if (t.pos() < n) keep.push_back(t);
        // every output takes the samples the cheapest way its placement allows: device rings straight from a device input
        // (rr_dstream_copy, no host hop), everything else through host memory (one download at most)
        const T* hp = nullptr;
        auto feed = [&](BufferWriter<T>& o) {
            if (input.device() && o.device()) { o.fill_from_device(input, n); return; }
            if (!hp) {
                if (input.device()) { bounce_.resize(n); input.copy_to(bounce_.data(), n); hp = bounce_.data(); }
                else hp = input.slice();
            }
            o.fill_from_slice(hp, n);
        };
        feed(o1);
        feed(o2);
        input.consume(n);
        o1.produce(n, keep);
        o2.produce(n, keep);
        return BlockRet::again();
    }
};

// SignalSourceComplex (src/signal_source.rs:9-63): amplitude * (sin(c), sin(c - pi/2)), the phase kept in
// f64 and wrapped with fmod each sample; fills the whole write window per work().
class SignalSourceComplex : public Block {
    WriteStream<Complex> dst_;
    Float amplitude_;
    double rad_per_sample_, current_ = 0.0;
    std::vector<Complex> tmp_;
public:
    SignalSourceComplex(WriteStream<Complex> dst, Float samp_rate, Float freq, Float amplitude)
        : dst_(std::move(dst)), amplitude_(amplitude),
          rad_per_sample_(2.0 * M_PI * (double)freq / (double)samp_rate) {
        if (!(samp_rate > 0.0f)) throw Error("SignalSourceComplex: samp_rate must be > 0");   // :26 assert
    }
    static std::pair<std::unique_ptr<SignalSourceComplex>, ReadStream<Complex>> new_(Float samp_rate, Float freq, Float amplitude) {
        auto [w, r] = new_stream<Complex>();
        return {std::make_unique<SignalSourceComplex>(std::move(w), samp_rate, freq, amplitude), std::move(r)};
    }
    const char* block_name() const override { return "SignalSourceComplex"; }
    bool eof() override { return false; }
    BlockRet work() override {                    // :55-63
        auto o = dst_.write_buf();
        const size_t n = o.len();
        tmp_.resize(n);
        for (size_t i = 0; i < n; i++) {          // Iterator::next, :41-52
            current_ = std::fmod(current_ + rad_per_sample_, 2.0 * M_PI);
            const Complex v((Float)std::sin(current_), (Float)std::sin(current_ - M_PI / 2.0));
            tmp_[i] = amplitude_ * v;
        }
        o.fill_from_slice(tmp_.data(), n);
        o.produce(n, {});
        return BlockRet::wait(dst_.wait_handle(), 1);
    }
};

// Single-threaded round-robin runner (src/graph.rs:99-173), minus timing statistics.  A block
// that reaches EOF is dropped, which closes its output streams (the reference: Arc strong
// count, src/stream.rs:148-150, 237-246); the run ends when a whole round moves no sample
// and returns no Again/Pending (src/graph.rs:108-154).
class Graph {
    std::vector<std::unique_ptr<Block>> blocks_;
public:
    void add(std::unique_ptr<Block> b) { blocks_.push_back(std::move(b)); }
    void run() {
        for (;;) {
            bool done = true;
            const uint64_t before = detail::activity();
            for (auto& bp : blocks_) {
                if (!bp) continue;
                const BlockRet ret = bp->work();
                switch (ret.kind) {
                case BlockRet::Again:
                case BlockRet::Pending: done = false; break;
                case BlockRet::EOF_: bp.reset(); done = false; break;
                case BlockRet::WaitForStream:
                    if (bp->eof() || ret.stream->closed()) { bp.reset(); done = false; }   // graph.rs:136-143
                    break;
                }
            }
            if (done && detail::activity() == before) break;
        }
    }
};


// Thread-per-block runner (src/mtgraph.rs:84-135).  Each block runs on its own thread until its work() says EOF, or says
// WaitForStream and either the block's own eof() holds or the stream's wait(need) reports that `need` can never be met
// (:109-115); Pending sleeps with a doubling back-off (:116-122).  The block is dropped when its thread ends, which closes
// its ends of its streams and so wakes and ends its neighbours.  A throwing work() cancels the graph (:99-105).
class MTGraph {
    std::vector<std::unique_ptr<Block>> blocks_;
public:
    void add(std::unique_ptr<Block> b) { blocks_.push_back(std::move(b)); }
    void run() {
        using namespace std::chrono;
        constexpr auto MIN_IDLE_SLEEP = microseconds(1000), MAX_IDLE_SLEEP = microseconds(100000);   // mtgraph.rs:14-15
        std::atomic<bool> cancel{false};
        std::mutex em;
        std::string err;
        std::vector<std::thread> threads;
        for (auto& slot : blocks_) {
            threads.emplace_back([&cancel, &em, &err, MIN_IDLE_SLEEP, MAX_IDLE_SLEEP, b = std::move(slot)]() mutable {
                auto idle = MIN_IDLE_SLEEP;
                bool running = true;
                while (running && !cancel.load()) {
                    BlockRet ret = BlockRet::again();
                    try {
                        ret = b->work();
                    } catch (const std::exception& e) {
                        std::lock_guard<std::mutex> g(em);
                        if (err.empty()) err = std::string("in block ") + b->block_name() + ": " + e.what();
                        cancel = true;
                        break;
                    }
                    switch (ret.kind) {
                    case BlockRet::Again: idle = MIN_IDLE_SLEEP; break;
                    case BlockRet::EOF_: running = false; break;
                    case BlockRet::WaitForStream: {
                        const bool never = ret.stream->wait(ret.need);
                        if (b->eof() || never) running = false;
                        break;
                    }
                    case BlockRet::Pending:
                        std::this_thread::sleep_for(idle);
                        idle = std::min(idle * 2, MAX_IDLE_SLEEP);
                        break;
                    }
                }
                b.reset();                                   // the drop that closes this block's stream ends
            });
        }
        blocks_.clear();
        for (auto& t : threads) t.join();
        if (!err.empty()) throw Error(err);
    }
};

}  // namespace rustradio
