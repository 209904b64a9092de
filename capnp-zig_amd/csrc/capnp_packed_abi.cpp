// capnp_packed_abi.cpp — the C-ABI boundary (include/capnp_packed.h).
//
// Conventions follow the reference's only FFI, src/wasm/capnp_host_abi.zig:
// integer status codes, a last-error message (:165-184), and a version query
// (:60-70). Single-buffer calls run ONE unit through the GPU via a small
// mutex-guarded device context; batch calls only enqueue kernels on the
// caller's stream. There is no CPU code path: without a gfx950 device every
// compute entry point returns CAPNP_PACKED_NO_DEVICE.
//
// How the file is laid out:
// - Buf is the one owner of device and page-locked memory. How a buffer grows (Growth) is data
//   of its call site; freeing is an explicit release(), never a destructor.
// - Every device scratch block has one definition that sizes it and hands out its typed parts
//   (UnitCols and its three blocks, StateBlock, RoundBlock, SpecBlock): reserve calls, copies
//   and launch arguments all take them from there.
// - The framer session's read (framer_read_locked) is a loop over named steps (append,
//   walk_pass, decode_pass, commit_pass); where its bytes live is planned in framer_layout.h,
//   which knows no HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "capnp_packed.h"
#include "class_ws.h"
#include "framer_layout.h"
#include "kernels.h"

namespace {

thread_local std::string g_last_error;

int fail(int status, const std::string& msg) {
    g_last_error = msg;
    return status;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(CAPNP_PACKED_DEVICE_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

// What a launcher or a chain of HIP calls returned, as a status.
int launched(hipError_t e, const char* what) { return e == hipSuccess ? CAPNP_PACKED_OK : hip_fail(e, what); }

std::once_flag g_init_once;
int g_init_status = CAPNP_PACKED_NO_DEVICE;
std::string g_init_error;

void device_init() {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_init_status = CAPNP_PACKED_NO_DEVICE;
        g_init_error = "no HIP device visible";
        return;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) {
        g_init_status = CAPNP_PACKED_DEVICE_ERROR;
        g_init_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_init_status = CAPNP_PACKED_NO_DEVICE;
        g_init_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return;
    }
    g_init_status = CAPNP_PACKED_OK;
}

int ensure_device() {
    std::call_once(g_init_once, device_init);
    if (g_init_status != CAPNP_PACKED_OK) return fail(g_init_status, g_init_error);
    return CAPNP_PACKED_OK;
}

// ---------------------------------------------------------------------------
// Buffers
// ---------------------------------------------------------------------------
// How a buffer grows: the bytes to allocate for a call that needs `need`, the label of a failed
// allocation, and whether a buffer grown by an unusually large call is given back on the next
// call that needs a quarter of it or less (above 64 MiB), so that its owner does not pin its
// peak for the process.
struct Growth {
    const char* what;
    uint64_t (*want)(uint64_t need);
    bool give_back;
};
uint64_t half_more_from_64k(uint64_t need) { return need < 65536 ? 65536 : need + need / 2; }
uint64_t half_more_min_4k(uint64_t need) { return std::max<uint64_t>(need + need / 2, 4096); }
uint64_t quarter_more_min_1m(uint64_t need) { return std::max<uint64_t>(need + need / 4, 1u << 20); }
uint64_t exactly(uint64_t need) { return need; }

constexpr Growth kSingleDevice{"hipMalloc(workspace)", half_more_from_64k, true};       // single-buffer calls
constexpr Growth kSingleStaging{"hipHostMalloc(staging)", half_more_from_64k, true};
constexpr Growth kFrameRounds{"hipMalloc(framer)", half_more_from_64k, false};          // frame_connections
constexpr Growth kSession{"hipMalloc(framer session)", half_more_from_64k, false};      // the framer session
constexpr Growth kSessionArena{"hipMalloc(framer arena)", exactly, false};
constexpr Growth kSessionMeta{"hipHostMalloc(framer metadata)", half_more_min_4k, false};
constexpr Growth kSessionStaging{"hipHostMalloc(framer staging)", quarter_more_min_1m, false};

// A device (hipMalloc) or page-locked host (hipHostMalloc) allocation and its size. reserve()
// keeps what holds `need` bytes and otherwise replaces it (the contents are not kept).
// There is no destructor: the process-lifetime contexts below (g_ctx, g_fr) never free, because
// at static destruction the HIP runtime may already be gone; every other owner calls release().
template <bool Pinned>
struct Buf {
    uint8_t* p = nullptr;
    uint64_t cap = 0;

    int reserve(uint64_t need, const Growth& g) {
        if (p && need <= cap && !(g.give_back && cap > (64u << 20) && need <= cap / 4)) return CAPNP_PACKED_OK;
        if (need > (SIZE_MAX / 3) * 2)  // g.want(need) stays inside size_t
            return fail(CAPNP_PACKED_OUT_OF_SPACE,
                        Pinned ? "staging size overflows size_t" : "workspace size overflows size_t");
        release();
        const uint64_t want = g.want(need);
        const hipError_t e = Pinned ? hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault)
                                    : hipMalloc(reinterpret_cast<void**>(&p), want);
        if (e != hipSuccess) {
            p = nullptr;
            return hip_fail(e, g.what);
        }
        cap = want;
        return CAPNP_PACKED_OK;
    }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};

// ---------------------------------------------------------------------------
// Scratch layouts. Each is a view (base pointer and counts) of a block on the device or of its
// host copy; the byte layout is the same on both sides.
// ---------------------------------------------------------------------------
// The metadata of n units, column after column (one u64 per unit each). Every block starts with
// the kernels' four inputs and out_len; the columns after them differ per block.
struct UnitCols {
    uint64_t* p;
    uint64_t n;
    uint64_t* col(uint32_t i) const { return p + i * n; }
    int32_t* col32(uint32_t i) const { return reinterpret_cast<int32_t*>(col(i)); }  // i32 in a u64 column
    uint64_t* in_off() const { return col(0); }
    uint64_t* in_len() const { return col(1); }
    uint64_t* out_off() const { return col(2); }
    uint64_t* out_cap() const { return col(3); }
    uint64_t* out_len() const { return col(4); }
    uint64_t inputs_bytes() const { return 4 * n * 8; }  // in_off .. out_cap: one H2D
};
// run_single's one unit: then status, consumed. The whole block crosses both ways.
struct SingleMeta : UnitCols {
    static constexpr uint64_t kBytes = 7 * 8, kAllocBytes = 8 * 8;
    explicit SingleMeta(uint64_t* base) : UnitCols{base, 1} {}
    int32_t* status() const { return col32(5); }
    uint64_t* consumed() const { return col(6); }
};
// A round of capnp_packed_frame_connections: then consumed, status.
struct RoundMeta : UnitCols {
    static uint64_t bytes(uint64_t n) { return 7 * n * 8; }
    uint64_t* consumed() const { return col(5); }
    int32_t* status() const { return col32(6); }
    uint64_t results_bytes() const { return 2 * n * 8 + n * 4; }  // out_len, consumed, status: one D2H
};
// A decode pass of the framer session: then status.
struct UnitBlock : UnitCols {
    static uint64_t host_bytes(uint64_t n) { return 6 * n * 8; }
    static uint64_t device_bytes(uint64_t n) { return host_bytes(n) + 64; }
    int32_t* status() const { return col32(5); }
    uint64_t results_bytes() const { return 2 * n * 8; }  // out_len and the status column: one D2H
};

// The framer session's state block: seven columns of n entries (u64 base, avail, need, X, W and
// a free slot; i32 status in the seventh).
// On the device a read's copy jobs live past the columns in the same allocation, and the jobs
// that append() enqueues without waiting are still being read when the read's first walk pass
// reserves the block for its columns. That reserve must not reallocate it. Both sizes come from
// device_bytes(): the pass asks for device_bytes(n, 0), never more than the device_bytes(n, jobs)
// the append asked for, and the buffer only grows.
// The host copy (page-locked) holds the pass's list (u32 per connection) past the columns.
struct StateBlock {
    uint8_t* p;
    uint64_t n;
    static uint64_t cols_bytes(uint64_t n) { return n * 56; }
    static uint64_t jobs_at(uint64_t n) { return cols_bytes(n) + 256; }
    static uint64_t device_bytes(uint64_t n, uint64_t job_bytes) { return jobs_at(n) + job_bytes + 64 * n + 4096; }
    static uint64_t host_bytes(uint64_t n) { return cols_bytes(n) + 4 * n; }
    uint64_t* col(uint32_t i) const { return reinterpret_cast<uint64_t*>(p) + i * n; }
    uint64_t* base() const { return col(0); }
    uint64_t* avail() const { return col(1); }
    uint64_t* need() const { return col(2); }
    uint64_t* X() const { return col(3); }
    uint64_t* W() const { return col(4); }
    int32_t* status() const { return reinterpret_cast<int32_t*>(col(6)); }
    uint64_t* jobs() const { return reinterpret_cast<uint64_t*>(p + jobs_at(n)); }  // device
    uint32_t* list() const { return reinterpret_cast<uint32_t*>(p + cols_bytes(n)); }  // host
    uint64_t inputs_bytes() const { return 5 * n * 8; }           // base .. W: one H2D
    uint64_t results_bytes() const { return 4 * n * 8 + 4 * n; }  // need, X, W, the free slot, status: one D2H
};

// A walk pass over k connections: the list, the count of messages found per connection, and the
// message table (M entries of packed length, framed length per connection), u32 each. The counts
// and the table come back as one copy.
struct RoundBlock {
    uint8_t* p;
    uint64_t k, M;
    static uint64_t tab_words(uint64_t k, uint64_t M) { return 2 * k * M; }
    static uint64_t device_bytes(uint64_t k, uint64_t M) { return 4 * (2 * k + tab_words(k, M)) + 256; }
    static uint64_t results_bytes(uint64_t k, uint64_t M) { return 4 * (k + tab_words(k, M)); }
    uint32_t* list() const { return reinterpret_cast<uint32_t*>(p); }
    uint32_t* counts() const { return list() + k; }
    uint32_t* table() const { return counts() + k; }
};
// Its results on the host: the counts, then the table.
struct RoundResults {
    const uint32_t* p;
    uint64_t k, M;
    uint32_t count(uint32_t j) const { return p[j]; }
    const uint32_t* messages(uint32_t j) const { return p + k + 2 * j * M; }  // packed, framed length per message
};

// The window tables of a walk pass over k connections with T windows in all: the tables' queue
// (cpk::framer_spec_bytes; its u64 at u32 index cpk::kSlotReserved is T), then per listed connection the first
// window and the count (u32), then its bytes' arena offset and length (u64). A pass without
// tables has p null, and every part of the block is null with it.
struct SpecBlock {
    uint8_t* p;
    uint64_t k, qb, ab;
    SpecBlock(uint32_t k_, uint64_t T)
        : p(nullptr), k(k_), qb((cpk::framer_spec_bytes(k_, T) + 15) & ~15ull), ab((8ull * k_ + 15) & ~15ull) {}
    uint64_t device_bytes() const { return qb + ab + 16 * k + 64; }
    template <class T>
    T* at(uint64_t byte, uint64_t i) const { return p ? reinterpret_cast<T*>(p + byte) + i : nullptr; }
    uint32_t* queue() const { return at<uint32_t>(0, 0); }
    uint32_t* windows() const { return at<uint32_t>(0, cpk::kSlotReserved); }
    uint32_t* first() const { return at<uint32_t>(qb, 0); }
    uint32_t* count() const { return at<uint32_t>(qb, k); }
    uint64_t* off() const { return at<uint64_t>(qb + ab, 0); }
    uint64_t* len() const { return at<uint64_t>(qb + ab, k); }
};

// Device context for the single-buffer host entry points: device buffers and pinned host
// staging (the caller's pageable bytes are copied into pinned memory, so the H2D / D2H copies
// run as DMA at full PCIe rate), one stream, the meta block's host copy in pinned memory too.
struct HostCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    Buf<false> d_in, d_out;
    Buf<true> h_in, h_out;
    uint64_t* d_meta = nullptr;  // SingleMeta
    uint64_t* h_meta = nullptr;

    int init() {
        if (stream) return CAPNP_PACKED_OK;
        hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
        e = hipMalloc(&d_meta, SingleMeta::kAllocBytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(meta)");
        e = hipHostMalloc(reinterpret_cast<void**>(&h_meta), SingleMeta::kAllocBytes, hipHostMallocDefault);
        return launched(e, "hipHostMalloc(meta)");
    }
};

HostCtx g_ctx;

// Device buffers of capnp_packed_frame_connections (grow-only; its own streams and lock,
// so framing never waits on a single-buffer call). Frame slots are double-buffered: round r
// decodes into d_out[r % 2] while the copy stream moves round r - 1's frames to the host.
struct FrameCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipStream_t copy = nullptr;   // frames D2H, overlapping the next round
    hipEvent_t ev_done[2] = {nullptr, nullptr};  // round into d_out[b] decoded
    hipEvent_t ev_copied[2] = {nullptr, nullptr};  // frames of d_out[b] on the host
    Buf<false> d_in, d_out[2], d_meta;

    int init() {
        if (stream) return CAPNP_PACKED_OK;
        hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking);
        for (int b = 0; b < 2 && e == hipSuccess; ++b) {
            e = hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_copied[b], hipEventDisableTiming);
        }
        return launched(e, "hipStreamCreate(framer)");
    }
};

FrameCtx g_fr;

// Largest unpacked size of n packed bytes: a 2-byte zero-run record expands to 256 words.
uint64_t unpack_bound(size_t n) { return n > (UINT64_MAX / 1024) ? UINT64_MAX : 1024ull * n; }

// Run one unit through a batch kernel (kReadMessage: reader.zig:84-156; *used_out = packed bytes
// consumed). The input crosses PCIe once (pinned staging), the kernels run with an output slot
// of `slot` bytes, and the output comes back only when the unit is OK; *len_out is out_len (for
// OUT_OF_SPACE: the size the unit needs).
// reuse_in: the device already holds `in` from the previous call (a retry with a larger slot).
// Single units up to these sizes take one kernel (cpk::launch_decode_one / launch_encode_one);
// DESIGN.md §6.1 has the measured crossover.
constexpr size_t kFastDecodeMax = 24 * 1024;  // packed bytes (the serial window walk passes the batch path near 32 KB)
constexpr size_t kFastEncodeMax = 4096;       // unpacked bytes: one 512-word tile

enum class Single { kEncode, kDecode, kDecodedSize, kEncodedSize, kReadMessage, kEncodeFramed };

int run_single(Single kind, const uint8_t* in, size_t n, uint8_t* out, size_t slot, uint64_t* len_out,
               uint64_t* used_out, bool reuse_in, uint32_t dialect) {
    int st = g_ctx.init();
    if (st) return st;
    if (n > SIZE_MAX - 16 || slot > SIZE_MAX - 16) return fail(CAPNP_PACKED_OUT_OF_SPACE, "buffer size overflows size_t");
    if (!reuse_in) {
        if ((st = g_ctx.d_in.reserve(n + 16, kSingleDevice))) return st;
        if ((st = g_ctx.h_in.reserve(n + 16, kSingleStaging))) return st;
    }
    const bool framed = kind == Single::kEncodeFramed;  // the C++ dialect's: a framed message, piece by piece
    const bool encodes = kind == Single::kEncode || kind == Single::kEncodedSize || framed;
    const bool write = kind == Single::kEncode || kind == Single::kDecode || kind == Single::kReadMessage || framed;
    if (write && (st = g_ctx.d_out.reserve(slot + 16, kSingleDevice))) return st;
    // one kernel for a single unit the one-unit kernels take (kFastDecodeMax / kFastEncodeMax)
    const bool one = n > 0 && ((kind == Single::kDecode && n <= kFastDecodeMax) || (encodes && n <= kFastEncodeMax));
    const SingleMeta hm(g_ctx.h_meta), m(g_ctx.d_meta);
    std::memset(hm.p, 0, SingleMeta::kBytes);
    *hm.in_len() = n;
    *hm.out_cap() = slot;
    // decode_wave_kernel<kWvMarked> takes marked units
    if (one && kind == Single::kDecode) *hm.status() = cpk::decode_one_status();
    hipStream_t s = g_ctx.stream;
    hipError_t e = hipSuccess;
    if (n && !reuse_in) {
        std::memcpy(g_ctx.h_in.p, in, n);
        e = hipMemcpyAsync(g_ctx.d_in.p, g_ctx.h_in.p, n, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(m.p, hm.p, SingleMeta::kBytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(H2D)");
    const uint8_t* const d_in = g_ctx.d_in.p;
    uint8_t* const d_out = g_ctx.d_out.p;
    if (one && kind == Single::kDecode)
        e = cpk::launch_decode_one(d_in, m.in_off(), m.in_len(), d_out, m.out_off(), m.out_cap(), m.out_len(),
                                   m.status(), s);
    else if (framed)
        e = cpk::launch_encode_framed(d_in, m.in_off(), m.in_len(), 1, d_out, m.out_off(), m.out_cap(), m.out_len(),
                                      m.status(), true, true, nullptr, s);
    else if (encodes && dialect == CAPNP_PACKED_DIALECT_CXX)
        e = cpk::launch_encode_cxx(d_in, m.in_off(), m.in_len(), 1, d_out, m.out_off(), m.out_cap(), m.out_len(),
                                   m.status(), write, s);
    else if (one)
        e = cpk::launch_encode_one(d_in, m.in_off(), m.in_len(), d_out, m.out_off(), m.out_cap(), m.out_len(),
                                   m.status(), write, s);
    else if (encodes)
        e = cpk::launch_encode(d_in, m.in_off(), m.in_len(), 1, d_out, m.out_off(), m.out_cap(), m.out_len(),
                               m.status(), write, nullptr, 0, s);
    else if (kind == Single::kReadMessage)
        e = cpk::launch_read_message(d_in, m.in_off(), m.in_len(), 1, d_out, m.out_off(), m.out_cap(), m.out_len(),
                                     m.consumed(), m.status(), s);
    else
        e = cpk::launch_decode(d_in, m.in_off(), m.in_len(), 1, d_out, m.out_off(), m.out_cap(), m.out_len(),
                               m.status(), write, nullptr, 0, s);
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    e = hipMemcpyAsync(hm.p, m.p, SingleMeta::kBytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(D2H)");
    const int32_t status = *hm.status();
    const uint64_t out_len = *hm.out_len();
    *len_out = out_len;
    if (used_out) *used_out = *hm.consumed();
    if (status == CAPNP_PACKED_OK && write && out_len) {
        const size_t len = (size_t)out_len;
        if ((st = g_ctx.h_out.reserve(len, kSingleStaging))) return st;
        e = hipMemcpyAsync(g_ctx.h_out.p, d_out, len, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(D2H out)");
        std::memcpy(out, g_ctx.h_out.p, len);
    }
    if (status != CAPNP_PACKED_OK) g_last_error = capnp_packed_status_name(status);
    return status;
}

// capnp_packed_encode / _dialect with the dialect known to be one of the two
int encode_single(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, uint32_t dialect) {
    if (!out_len) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "out_len is null");
    *out_len = 0;
    if ((n && !in) || (cap && !out)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null buffer");
    if (n % 8) return fail(CAPNP_PACKED_INVALID_MESSAGE_SIZE, "InvalidMessageSize");  // message.zig:201
    int st = ensure_device();
    if (st) return st;
    std::lock_guard<std::mutex> lock(g_ctx.mu);
    size_t bound = capnp_packed_encode_bound(n);
    uint64_t len = 0;
    st = run_single(Single::kEncode, in, n, out, cap < bound ? cap : bound, &len, nullptr, false, dialect);
    *out_len = (size_t)len;
    return st;
}

// The per-unit checks of the framed calls on host bytes (the kernels' framed_parse): Message.init's
// table parse (message.zig:341-394), then the exact-length rule.
int framed_verdict(const uint8_t* in, size_t n) {
    if (n % 8) return CAPNP_PACKED_INVALID_MESSAGE_SIZE;
    if (n < 4) return CAPNP_PACKED_END_OF_STREAM;
    uint32_t m1;
    std::memcpy(&m1, in, 4);
    if (m1 == 0xFFFFFFFFu) return CAPNP_PACKED_INVALID_SEGMENT_COUNT;
    if (m1 >= 512u) return CAPNP_PACKED_SEGMENT_COUNT_LIMIT_EXCEEDED;
    const uint64_t count = (uint64_t)m1 + 1, hw = count / 2 + 1;
    if (8 * hw > n) return CAPNP_PACKED_TRUNCATED_MESSAGE;
    uint64_t total = hw;
    for (uint64_t s = 0; s < count; ++s) {
        uint32_t sw;
        std::memcpy(&sw, in + 4 + 4 * s, 4);
        total += sw;
    }
    if (total > n / 8) return CAPNP_PACKED_TRUNCATED_MESSAGE;
    if (total < n / 8) return CAPNP_PACKED_INVALID_ARGUMENT;  // trailing words
    if (n / 8 > 0xFFFFF000ull) return CAPNP_PACKED_INVALID_ARGUMENT;
    return CAPNP_PACKED_OK;
}

int check_dialect(uint32_t dialect) {
    if (dialect != CAPNP_PACKED_DIALECT_ZIG && dialect != CAPNP_PACKED_DIALECT_CXX)
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "unknown dialect");
    return CAPNP_PACKED_OK;
}

int check_batch(const uint64_t* d_in_off, const uint64_t* d_in_len, uint32_t n, const uint64_t* d_len,
                const int32_t* d_status) {
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_in_off || !d_in_len || !d_len || !d_status) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    return ensure_device();
}

// The kernels address the workspace as u32 counters, 16-B table entries and 64-B
// record stores at 256-B offsets: it must be 256-B aligned (hipMalloc's alignment).
int check_ws(const void* ws, size_t bytes, size_t required, const char* too_small) {
    if (!ws) return CAPNP_PACKED_OK;
    if (reinterpret_cast<uintptr_t>(ws) & 255)
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "workspace not 256-B aligned");
    if (bytes < required) return fail(CAPNP_PACKED_INVALID_ARGUMENT, too_small);
    return CAPNP_PACKED_OK;
}
int check_queue_ws(const void* ws, size_t bytes, uint32_t n) {
    return check_ws(ws, bytes, cpk::queue_bytes(n), "workspace smaller than capnp_packed_batch_workspace_bytes(n)");
}

// A batch through cpk::launch_encode or launch_decode with an optional caller workspace
// (write = false: sizes only, no output arrays).
int codec_batch(decltype(&cpk::launch_encode) launch, const char* what, const uint8_t* d_in, const uint64_t* d_in_off,
                const uint64_t* d_in_len, uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status, bool write, void* d_workspace,
                size_t workspace_bytes, void* stream) {
    int st = check_batch(d_in_off, d_in_len, n, d_out_len, d_status);
    if (st || n == 0) return st;
    if (write && (!d_out_off || !d_out_cap)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output slot arrays");
    if ((st = check_queue_ws(d_workspace, workspace_bytes, n))) return st;
    return launched(launch(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status, write,
                           d_workspace, workspace_bytes, static_cast<hipStream_t>(stream)),
                    what);
}

// capnp_packed_encode_message_batch / _dialect with the dialect known to be one of the two
int encode_message_batch(const uint64_t* d_seg_ptr, const uint64_t* d_seg_len, const uint32_t* d_seg_first,
                         const uint32_t* d_seg_count, uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                         const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status, bool cxx, void* stream) {
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_seg_first || !d_seg_count || !d_out_len || !d_status)
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    const bool write = d_out != nullptr;
    if (write && (!d_out_off || !d_out_cap)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output slot arrays");
    int st = ensure_device();
    if (st) return st;
    const auto launch = cxx ? cpk::launch_encode_message_cxx : cpk::launch_encode_message;
    return launched(launch(d_seg_ptr, d_seg_len, d_seg_first, d_seg_count, n, d_out, d_out_off, d_out_cap, d_out_len,
                           d_status, write, static_cast<hipStream_t>(stream)),
                    "encode-message launch");
}

// capnp_packed_encode_dense_batch and capnp_packed_encode_framed_dense_batch. Every argument
// check answers before any device work.
int encode_dense_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, uint32_t n,
                       uint8_t* d_out, uint64_t out_base, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_out_len,
                       int32_t* d_status, uint32_t dialect, void* d_workspace, size_t workspace_bytes, void* stream,
                       bool framed, const char* what) {
    if (int st = check_dialect(dialect)) return st;
    if (n == 0 && !d_out_off) return CAPNP_PACKED_OK;
    if (n) {
        if (!d_in_off || !d_in_len || !d_out_off || !d_out_len || !d_status)
            return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
        if (!d_workspace) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "the dense encode needs a workspace");
        int st = check_ws(d_workspace, workspace_bytes, cpk::dense_workspace_bytes(n),
                          "workspace smaller than capnp_packed_encode_dense_workspace_bytes(n)");
        if (st) return st;
    }
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_encode_dense(d_in, d_in_off, d_in_len, n, d_out, out_base, out_cap, d_out_off,
                                             d_out_len, d_status, dialect == CAPNP_PACKED_DIALECT_CXX, framed,
                                             d_workspace, static_cast<hipStream_t>(stream)),
                    what);
}

}  // namespace

extern "C" {

uint32_t capnp_packed_abi_version(void) { return CAPNP_PACKED_ABI_VERSION; }

const char* capnp_packed_last_error(void) { return g_last_error.c_str(); }

const char* capnp_packed_status_name(int status) {
    switch (status) {
        case CAPNP_PACKED_OK: return "Ok";
        case CAPNP_PACKED_INVALID_MESSAGE_SIZE: return "InvalidMessageSize";
        case CAPNP_PACKED_UNEXPECTED_EOF: return "UnexpectedEof";
        case CAPNP_PACKED_OVERFLOW: return "Overflow";
        case CAPNP_PACKED_OUT_OF_SPACE: return "OutOfSpace";
        case CAPNP_PACKED_INVALID_ARGUMENT: return "InvalidArgument";
        case CAPNP_PACKED_DEVICE_ERROR: return "DeviceError";
        case CAPNP_PACKED_NO_DEVICE: return "NoDevice";
        case CAPNP_PACKED_END_OF_STREAM: return "EndOfStream";
        case CAPNP_PACKED_INVALID_SEGMENT_COUNT: return "InvalidSegmentCount";
        case CAPNP_PACKED_SEGMENT_COUNT_LIMIT_EXCEEDED: return "SegmentCountLimitExceeded";
        case CAPNP_PACKED_MESSAGE_TOO_LARGE: return "MessageTooLarge";
        case CAPNP_PACKED_INVALID_PACKED_MESSAGE: return "InvalidPackedMessage";
        case CAPNP_PACKED_TRUNCATED_MESSAGE: return "TruncatedMessage";
        case CAPNP_PACKED_EMPTY_MESSAGE: return "EmptyMessage";
        case CAPNP_PACKED_NESTING_LIMIT_EXCEEDED: return "NestingLimitExceeded";
        case CAPNP_PACKED_INVALID_SEGMENT_ID: return "InvalidSegmentId";
        case CAPNP_PACKED_INVALID_POINTER: return "InvalidPointer";
        case CAPNP_PACKED_OUT_OF_BOUNDS: return "OutOfBounds";
        case CAPNP_PACKED_TRAVERSAL_LIMIT_EXCEEDED: return "TraversalLimitExceeded";
        case CAPNP_PACKED_INVALID_FAR_POINTER: return "InvalidFarPointer";
        case CAPNP_PACKED_INVALID_INLINE_COMPOSITE_POINTER: return "InvalidInlineCompositePointer";
        case CAPNP_PACKED_LIST_TOO_LARGE: return "ListTooLarge";
        default: return "Unknown";
    }
}

size_t capnp_packed_encode_bound(size_t n) { return 10 * (n / 8); }

int capnp_packed_encode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len) {
    return encode_single(in, n, out, cap, out_len, CAPNP_PACKED_DIALECT_ZIG);
}

int capnp_packed_encode_dialect(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                                uint32_t dialect) {
    if (int st = check_dialect(dialect)) return st;
    return encode_single(in, n, out, cap, out_len, dialect);
}

int capnp_packed_decoded_size(const uint8_t* in, size_t n, size_t* out_size) {
    if (!out_size) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "out_size is null");
    *out_size = 0;
    if (n && !in) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null buffer");
    int st = ensure_device();
    if (st) return st;
    std::lock_guard<std::mutex> lock(g_ctx.mu);
    uint64_t len = 0;
    st = run_single(Single::kDecodedSize, in, n, nullptr, 0, &len, nullptr, false, CAPNP_PACKED_DIALECT_ZIG);
    if (st == CAPNP_PACKED_OK) *out_size = (size_t)len;
    return st;
}

int capnp_packed_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len) {
    if (!out_len) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "out_len is null");
    *out_len = 0;
    if ((n && !in) || (cap && !out)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null buffer");
    int st = ensure_device();
    if (st) return st;
    std::lock_guard<std::mutex> lock(g_ctx.mu);
    // One H2D and one decode into a device slot of min(cap, 8 n, at least 64 KiB) bytes: dense
    // data expands ~1.1-2x, so that slot nearly always holds it, and a large reusable caller
    // buffer does not size the device slot (up to 1024 n). A unit that does not fit ends
    // OUT_OF_SPACE with its size in out_len (the output is copied back only when OK, so the
    // caller's buffer is untouched, message.zig:90); if the caller's capacity holds that size
    // the decode runs again from the input already on the device, into a slot of that size.
    const uint64_t bound = unpack_bound(n);
    const uint64_t room = cap < bound ? cap : bound;
    const uint64_t guess = n > (UINT64_MAX / 8) ? UINT64_MAX : (8ull * n < 65536 ? 65536 : 8ull * n);
    const uint64_t first = room < guess ? room : guess;
    uint64_t len = 0;
    st = run_single(Single::kDecode, in, n, out, (size_t)first, &len, nullptr, false, CAPNP_PACKED_DIALECT_ZIG);
    if (st == CAPNP_PACKED_OUT_OF_SPACE && first < room && len <= room)
        st = run_single(Single::kDecode, in, n, out, (size_t)len, &len, nullptr, true, CAPNP_PACKED_DIALECT_ZIG);
    *out_len = (st == CAPNP_PACKED_OK || st == CAPNP_PACKED_OUT_OF_SPACE) ? (size_t)len : 0;
    return st;
}

size_t capnp_packed_batch_workspace_bytes(uint32_t n) { return cpk::queue_bytes(n); }

int capnp_packed_set_decoder(int decoder) {
    if (decoder < CAPNP_PACKED_DECODER_AUTO || decoder > CAPNP_PACKED_DECODER_WORDS)
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "unknown decoder");
    if (!cpk::decoder_built(decoder))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "decoder removed from the library (round 5; DESIGN.md §2.3a, §2.3b)");
    return cpk::set_decoder(decoder);
}

int capnp_packed_set_all_or_nothing(int on) { return cpk::set_all_or_nothing(on); }

uint32_t capnp_packed_set_launch_flags(uint32_t flags) {
    return cpk::set_launch_flags(flags & (CAPNP_PACKED_LAUNCH_LONG_INLINE | CAPNP_PACKED_LAUNCH_MID_SIDE_STREAM |
                                          CAPNP_PACKED_LAUNCH_CLASS_SCAN));
}

int capnp_packed_stream_release(void* stream) {
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::release_stream(static_cast<hipStream_t>(stream)), "stream release");
}

int capnp_packed_stream_queue_info(void* stream, size_t* bytes, uint32_t* kept) {
    if (!bytes || !kept) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output");
    *bytes = 0;
    *kept = 0;
    int st = ensure_device();
    if (st) return st;
    cpk::stream_queue_info(static_cast<hipStream_t>(stream), bytes, kept);
    return CAPNP_PACKED_OK;
}

int capnp_packed_stream_contexts(uint32_t* count) {
    if (!count) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output");
    *count = 0;
    int st = ensure_device();
    if (st) return st;
    *count = cpk::stream_context_count();
    return CAPNP_PACKED_OK;
}

int capnp_packed_encode_batch_ws(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                 uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                 uint64_t* d_out_len, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                                 void* stream) {
    return codec_batch(cpk::launch_encode, "encode launch", d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap,
                       d_out_len, d_status, true, d_workspace, workspace_bytes, stream);
}

int capnp_packed_encode_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                              uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                              uint64_t* d_out_len, int32_t* d_status, void* stream) {
    return capnp_packed_encode_batch_ws(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                                        d_status, nullptr, 0, stream);
}

int capnp_packed_encode_batch_dialect(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                      uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                      const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                      uint32_t dialect, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int st = check_dialect(dialect)) return st;
    if (dialect == CAPNP_PACKED_DIALECT_ZIG) {
        if (d_out)
            return capnp_packed_encode_batch_ws(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                                                d_status, d_workspace, workspace_bytes, stream);
        // sizes only: capnp_packed_encoded_size_batch with the caller's workspace
        return codec_batch(cpk::launch_encode, "encode-size launch", d_in, d_in_off, d_in_len, n, nullptr, nullptr,
                           nullptr, d_out_len, d_status, false, d_workspace, workspace_bytes, stream);
    }
    int st = check_batch(d_in_off, d_in_len, n, d_out_len, d_status);
    if (st || n == 0) return st;
    const bool write = d_out != nullptr;
    if (write && (!d_out_off || !d_out_cap)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output slot arrays");
    if ((st = check_queue_ws(d_workspace, workspace_bytes, n))) return st;  // checked, not used: one kernel
    return launched(cpk::launch_encode_cxx(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                                           d_status, write, static_cast<hipStream_t>(stream)),
                    "encode launch");
}

size_t capnp_packed_encode_dense_workspace_bytes(uint32_t n) { return cpk::dense_workspace_bytes(n); }

int capnp_packed_encode_dense_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint8_t* d_out, uint64_t out_base, uint64_t out_cap,
                                    uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, uint32_t dialect,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    return encode_dense_batch(d_in, d_in_off, d_in_len, n, d_out, out_base, out_cap, d_out_off, d_out_len, d_status,
                              dialect, d_workspace, workspace_bytes, stream, false, "dense encode launch");
}

int capnp_packed_encode_framed(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                               uint32_t dialect) {
    if (int st = check_dialect(dialect)) return st;
    if (!out_len) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "out_len is null");
    *out_len = 0;
    if ((n && !in) || (cap && !out)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null buffer");
    if (dialect == CAPNP_PACKED_DIALECT_ZIG) {
        // the framing only adds the checks: on the host's bytes, then packPacked(unit)
        const int v = framed_verdict(in, n);
        if (v != CAPNP_PACKED_OK) return fail(v, capnp_packed_status_name(v));
        return encode_single(in, n, out, cap, out_len, dialect);
    }
    if (n % 8) return fail(CAPNP_PACKED_INVALID_MESSAGE_SIZE, "InvalidMessageSize");
    int st = ensure_device();
    if (st) return st;
    std::lock_guard<std::mutex> lock(g_ctx.mu);
    const size_t bound = capnp_packed_encode_bound(n);
    uint64_t len = 0;
    st = run_single(Single::kEncodeFramed, in, n, out, cap < bound ? cap : bound, &len, nullptr, false, dialect);
    *out_len = (size_t)len;
    return st;
}

size_t capnp_packed_encode_framed_workspace_bytes(uint32_t n) { return cpk::framed_workspace_bytes(n); }

// Every argument check answers before any device work.
int capnp_packed_encode_framed_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                     uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                     const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                     uint32_t dialect, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int st = check_dialect(dialect)) return st;
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_in_off || !d_in_len || !d_out_len || !d_status)
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    const bool write = d_out != nullptr;
    if (write && (!d_out_off || !d_out_cap)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output slot arrays");
    if (!d_workspace) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "the framed encode needs a workspace");
    int st = check_ws(d_workspace, workspace_bytes, cpk::framed_workspace_bytes(n),
                      "workspace smaller than capnp_packed_encode_framed_workspace_bytes(n)");
    if (st) return st;
    if ((st = ensure_device())) return st;
    return launched(cpk::launch_encode_framed(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                                              d_status, write, dialect == CAPNP_PACKED_DIALECT_CXX, d_workspace,
                                              static_cast<hipStream_t>(stream)),
                    "framed encode launch");
}

int capnp_packed_encode_framed_dense_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                           uint32_t n, uint8_t* d_out, uint64_t out_base, uint64_t out_cap,
                                           uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status,
                                           uint32_t dialect, void* d_workspace, size_t workspace_bytes,
                                           void* stream) {
    return encode_dense_batch(d_in, d_in_off, d_in_len, n, d_out, out_base, out_cap, d_out_off, d_out_len, d_status,
                              dialect, d_workspace, workspace_bytes, stream, true, "framed dense encode launch");
}

size_t capnp_packed_split_workspace_bytes(uint32_t n, uint64_t in_bytes_bound) {
    return cpk::split_workspace_bytes(n, in_bytes_bound);
}

// Every argument check answers before any device work.
int capnp_packed_split_streams(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, uint32_t n,
                               uint64_t max_msgs, uint64_t* d_msg_first, uint64_t* d_msg_off, uint64_t* d_msg_len,
                               uint64_t* d_msg_framed, uint32_t* d_msg_stream, uint64_t* d_consumed,
                               int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!d_msg_first) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null d_msg_first");
    if (n) {
        if (!d_in_off || !d_in_len || !d_consumed || !d_status)
            return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
        if (max_msgs && (!d_msg_off || !d_msg_len || !d_msg_framed))
            return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null message table");
        if (!d_workspace) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "the splitter needs a workspace");
        int st = check_ws(d_workspace, workspace_bytes, cpk::split_workspace_bytes(n, 0),
                          "workspace smaller than capnp_packed_split_workspace_bytes(n, 0)");
        if (st) return st;
    }
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_split_streams(d_in, d_in_off, d_in_len, n, max_msgs, d_msg_first, d_msg_off, d_msg_len,
                                              d_msg_framed, d_msg_stream, d_consumed, d_status, d_workspace,
                                              workspace_bytes, static_cast<hipStream_t>(stream)),
                    "split launch");
}

int capnp_packed_encoded_size_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint64_t* d_out_len, int32_t* d_status, void* stream) {
    return codec_batch(cpk::launch_encode, "encode-size launch", d_in, d_in_off, d_in_len, n, nullptr, nullptr, nullptr,
                       d_out_len, d_status, false, nullptr, 0, stream);
}

int capnp_packed_decode_batch_ws(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                 uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                 uint64_t* d_out_len, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                                 void* stream) {
    return codec_batch(cpk::launch_decode, "decode launch", d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap,
                       d_out_len, d_status, true, d_workspace, workspace_bytes, stream);
}

int capnp_packed_decode_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                              uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                              uint64_t* d_out_len, int32_t* d_status, void* stream) {
    return capnp_packed_decode_batch_ws(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                                        d_status, nullptr, 0, stream);
}

int capnp_packed_decoded_size_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint64_t* d_out_len, int32_t* d_status, void* stream) {
    return codec_batch(cpk::launch_decode, "decode-size launch", d_in, d_in_off, d_in_len, n, nullptr, nullptr, nullptr,
                       d_out_len, d_status, false, nullptr, 0, stream);
}

int capnp_packed_read_message_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                    const uint64_t* d_out_cap, uint64_t* d_out_len, uint64_t* d_consumed,
                                    int32_t* d_status, void* stream) {
    int st = check_batch(d_in_off, d_in_len, n, d_out_len, d_status);
    if (st || n == 0) return st;
    if (!d_out_off || !d_out_cap || !d_consumed) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null output arrays");
    return launched(cpk::launch_read_message(d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                                             d_consumed, d_status, static_cast<hipStream_t>(stream)),
                    "read-message launch");
}

int capnp_packed_read_message(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                              size_t* consumed) {
    if (!out_len || !consumed) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "out_len/consumed is null");
    *out_len = 0;
    *consumed = 0;
    if ((n && !in) || (cap && !out)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null buffer");
    int st = ensure_device();
    if (st) return st;
    std::lock_guard<std::mutex> lock(g_ctx.mu);
    // reader.zig can produce at most a 512-segment header (257 words) plus
    // max_total_words (8 Mi, reader.zig:6) words: a larger cap is clamped, so the
    // device slot is sized by what the reader can write, not by the caller's buffer
    const size_t kMaxFramed = (257ull + 8ull * 1024 * 1024) * 8;
    uint64_t len = 0, used = 0;
    st = run_single(Single::kReadMessage, in, n, out, cap < kMaxFramed ? cap : kMaxFramed, &len, &used, false,
                    CAPNP_PACKED_DIALECT_ZIG);
    *out_len = (size_t)len;
    *consumed = (size_t)used;
    return st;
}

int capnp_packed_encode_message_batch(const uint64_t* d_seg_ptr, const uint64_t* d_seg_len,
                                      const uint32_t* d_seg_first, const uint32_t* d_seg_count, uint32_t n,
                                      uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                      uint64_t* d_out_len, int32_t* d_status, void* stream) {
    return encode_message_batch(d_seg_ptr, d_seg_len, d_seg_first, d_seg_count, n, d_out, d_out_off, d_out_cap,
                                d_out_len, d_status, false, stream);
}

int capnp_packed_encode_message_batch_dialect(const uint64_t* d_seg_ptr, const uint64_t* d_seg_len,
                                              const uint32_t* d_seg_first, const uint32_t* d_seg_count, uint32_t n,
                                              uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                              uint64_t* d_out_len, int32_t* d_status, uint32_t dialect,
                                              void* stream) {
    if (int st = check_dialect(dialect)) return st;
    return encode_message_batch(d_seg_ptr, d_seg_len, d_seg_first, d_seg_count, n, d_out, d_out_off, d_out_cap,
                                d_out_len, d_status, dialect == CAPNP_PACKED_DIALECT_CXX, stream);
}

int capnp_packed_message_init_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint32_t max_segs, uint32_t* d_seg_count, uint64_t* d_seg_off,
                                    uint64_t* d_seg_len, int32_t* d_status, void* stream) {
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_in_off || !d_in_len || !d_seg_count || !d_status || (max_segs && (!d_seg_off || !d_seg_len)))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_message_init(d_in, d_in_off, d_in_len, n, max_segs, d_seg_count, d_seg_off, d_seg_len,
                                             d_status, static_cast<hipStream_t>(stream)),
                    "message-init launch");
}

int capnp_packed_validate_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                uint32_t n, uint64_t segment_count_limit, uint64_t traversal_limit_words,
                                uint32_t nesting_limit, int32_t* d_status, uint64_t* d_words, void* stream) {
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_in_off || !d_in_len || !d_status) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_validate(d_in, d_in_off, d_in_len, n, segment_count_limit, traversal_limit_words,
                                         nesting_limit, d_status, d_words, static_cast<hipStream_t>(stream)),
                    "validate launch");
}

// what every field descriptor must satisfy, for a root read and an element read alike
static int check_field(const capnp_packed_field& a) {
    if (a.kind > CAPNP_PACKED_FIELD_LIST_64) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "unknown field kind");
    if (a.bit > (a.kind == CAPNP_PACKED_FIELD_BOOL ? 7u : 0u))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "bit is 0-7 for BOOL and 0 otherwise");
    if (a.path_len > CAPNP_PACKED_MAX_PATH) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "path longer than 4");
    return CAPNP_PACKED_OK;
}

int capnp_packed_read_fields_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                   uint32_t n, const capnp_packed_field* fields, uint32_t n_fields,
                                   uint64_t* d_value, uint64_t* d_len, uint64_t* d_count, int32_t* d_status,
                                   void* stream) {
    if (n_fields > CAPNP_PACKED_MAX_FIELDS) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "more than 32 fields");
    if (n == 0 || n_fields == 0) return CAPNP_PACKED_OK;
    if (!fields || !d_in || !d_in_off || !d_in_len || !d_value || !d_len || !d_status)
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    for (uint32_t f = 0; f < n_fields; ++f)
        if (int st = check_field(fields[f])) return st;
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_read_fields(d_in, d_in_off, d_in_len, n, fields, n_fields, d_value, d_len, d_count,
                                            d_status, static_cast<hipStream_t>(stream)),
                    "read-fields launch");
}

int capnp_packed_gather_batch(const uint8_t* d_in, const uint64_t* d_src_off, const uint64_t* d_src_len, uint32_t n,
                              uint8_t* d_out, const uint64_t* d_dst_off, uint64_t out_cap, int32_t* d_status,
                              void* stream) {
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_src_off || !d_src_len || !d_dst_off || !d_status || (out_cap && (!d_in || !d_out)))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_gather(d_in, d_src_off, d_src_len, n, d_out, d_dst_off, out_cap, d_status,
                                       static_cast<hipStream_t>(stream)),
                    "gather launch");
}

int capnp_packed_list_heads_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, uint32_t n,
                                  const uint32_t* path, uint32_t path_len, uint32_t pointer_index,
                                  uint32_t list_kind, capnp_packed_list_head* d_head, uint64_t* d_count,
                                  int32_t* d_status, void* stream) {
    if (list_kind > CAPNP_PACKED_LIST_POINTER) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "unknown list kind");
    if (path_len > CAPNP_PACKED_MAX_PATH) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "path longer than 4");
    if (n == 0) return CAPNP_PACKED_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_head || !d_count || !d_status || (path_len && !path))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_list_heads(d_in, d_in_off, d_in_len, n, path, path_len, pointer_index, list_kind,
                                           d_head, d_count, d_status, static_cast<hipStream_t>(stream)),
                    "list-heads launch");
}

int capnp_packed_read_elements_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                     uint32_t n, const capnp_packed_list_head* d_head, const uint64_t* d_elem_start,
                                     uint32_t list_kind, uint64_t elem_cap, const capnp_packed_field* fields,
                                     uint32_t n_fields, uint32_t* d_parent, uint32_t* d_index, uint64_t* d_value,
                                     uint64_t* d_len, uint64_t* d_count, int32_t* d_status, void* stream) {
    if (list_kind > CAPNP_PACKED_LIST_POINTER) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "unknown list kind");
    if (elem_cap >= (1ull << 32)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "elem_cap of 2^32 or more");
    if (n_fields > CAPNP_PACKED_MAX_FIELDS) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "more than 32 fields");
    if (n == 0 || elem_cap == 0) return CAPNP_PACKED_OK;
    if (n_fields == 0) {  // the element numbering only
        if (!d_parent && !d_index) return CAPNP_PACKED_OK;
        if (!d_elem_start) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    } else {
        if (!fields || !d_in || !d_in_off || !d_in_len || !d_head || !d_elem_start || !d_value || !d_len || !d_status)
            return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
        for (uint32_t f = 0; f < n_fields; ++f) {
            const capnp_packed_field& a = fields[f];
            if (int st = check_field(a)) return st;
            if (list_kind == CAPNP_PACKED_LIST_POINTER) {  // the element is one pointer
                if (a.path_len == 0 && a.kind <= CAPNP_PACKED_FIELD_BOOL)
                    return fail(CAPNP_PACKED_INVALID_ARGUMENT, "a pointer-list element has no data section");
                if (a.path_len == 0 && a.offset != 0)
                    return fail(CAPNP_PACKED_INVALID_ARGUMENT, "a pointer-list element has pointer 0 only");
                if (a.path_len && a.path[0] != 0)
                    return fail(CAPNP_PACKED_INVALID_ARGUMENT, "a pointer-list element has pointer 0 only");
            }
        }
    }
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_read_elements(d_in, d_in_off, n, d_head, d_elem_start, list_kind, elem_cap, fields,
                                              n_fields, d_parent, d_index, d_value, d_len, d_count, d_status,
                                              static_cast<hipStream_t>(stream)),
                    "read-elements launch");
}

int capnp_packed_build_fields_batch(const uint8_t* d_pool, uint64_t pool_len, uint32_t n,
                                    const capnp_packed_build_op* ops, uint32_t n_ops, const uint64_t* d_value,
                                    const uint64_t* d_len, const uint64_t* d_count, uint8_t* d_out,
                                    const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                    int32_t* d_status, void* stream) {
    if (n_ops > CAPNP_PACKED_MAX_BUILD_OPS) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "more than 32 build ops");
    if (n == 0) return CAPNP_PACKED_OK;
    cpk::SbPlan plan;
    if (const char* why = cpk::sb_compile(ops, n_ops, &plan)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, why);
    if (!d_value || !d_len || !d_out_len || !d_status || (d_out && (!d_out_off || !d_out_cap)) ||
        (pool_len && !d_pool))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null batch pointer");
    if (plan.has_bits && !d_count) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "d_count is null with a LIST_BIT op");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_build_fields(d_pool, pool_len, n, plan, d_value, d_len, d_count, d_out, d_out_off,
                                             d_out_cap, d_out_len, d_status, static_cast<hipStream_t>(stream)),
                    "build-fields launch");
}

size_t capnp_packed_scan_scratch_bytes(uint32_t n) { return cpk::scan_scratch_bytes(n); }

int capnp_packed_lengths_to_offsets(const uint64_t* d_len, uint32_t n, uint64_t base, uint64_t* d_off,
                                    void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!d_off || !d_scratch || (n && !d_len)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    if (scratch_bytes < cpk::scan_scratch_bytes(n)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "scratch too small");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_scan(d_len, n, base, d_off, static_cast<uint64_t*>(d_scratch),
                                     static_cast<hipStream_t>(stream)),
                    "scan launch");
}

int capnp_packed_generate(uint8_t* d_out, uint64_t n_units, uint64_t unit_bytes, uint64_t unit_base,
                          uint64_t seed, uint32_t zero_thresh, void* stream) {
    if (!d_out && n_units) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null d_out");
    if (unit_bytes % 8) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "unit_bytes % 8 != 0");
    int st = ensure_device();
    if (st) return st;
    return launched(cpk::launch_generate(d_out, n_units, unit_bytes, unit_base, seed, zero_thresh,
                                         static_cast<hipStream_t>(stream)),
                    "generate launch");
}

int capnp_packed_frame_connections(const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                                   const uint64_t* in_len, uint32_t n, uint64_t* slot_guess, uint8_t* frames,
                                   uint64_t frames_cap, uint64_t* frame_off, uint64_t* frame_len,
                                   uint32_t* frame_conn, uint32_t max_frames, uint64_t* consumed, int32_t* status,
                                   uint32_t* n_frames) {
    if (!n_frames) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "n_frames is null");
    *n_frames = 0;
    if (n == 0) return CAPNP_PACKED_OK;
    if (!in_off || !in_len || !slot_guess || !consumed || !status || (in_bytes && !in) ||
        (max_frames && (!frame_off || !frame_len || !frame_conn)) || (frames_cap && !frames))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    for (uint32_t c = 0; c < n; ++c)
        if (in_off[c] > in_bytes || in_len[c] > in_bytes - in_off[c])
            return fail(CAPNP_PACKED_INVALID_ARGUMENT, "connection bytes outside the input buffer");
    int st = ensure_device();
    if (st) return st;
    std::lock_guard<std::mutex> lock(g_fr.mu);
    if ((st = g_fr.init())) return st;
    // no copy of an earlier call may still write into its caller's frames buffer: each call
    // ends with the copy stream drained (copies_done below), also on its error paths
    struct CopiesDone {
        ~CopiesDone() { (void)hipStreamSynchronize(g_fr.copy); }
    } copies_done;
    if ((st = g_fr.d_in.reserve(in_bytes + 16, kFrameRounds))) return st;
    if ((st = g_fr.d_meta.reserve(RoundMeta::bytes(n), kFrameRounds))) return st;
    const hipStream_t s = g_fr.stream;
    hipError_t e = in_bytes ? hipMemcpyAsync(g_fr.d_in.p, in, in_bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(H2D input)");
    std::vector<uint64_t> used(n, 0), cap(n), meta(RoundMeta::bytes(n) / 8);
    std::vector<uint32_t> idx(n);
    std::vector<uint8_t> live(n);
    for (uint32_t c = 0; c < n; ++c) {
        live[c] = in_len[c] > 0;
        cap[c] = slot_guess[c] < 8 ? 8 : slot_guess[c];
        status[c] = CAPNP_PACKED_END_OF_STREAM;
    }
    uint64_t fcur = 0;  // bytes of `frames` used by earlier rounds
    uint32_t nf = 0;
    for (uint32_t r = 0;; ++r) {
        const uint32_t b = r & 1;  // this round's frame slots: d_out[b]
        // one round: the next message of every connection that may still hold one
        uint32_t k = 0;
        for (uint32_t c = 0; c < n; ++c)
            if (live[c] && used[c] < in_len[c]) idx[k++] = c;
        if (k == 0) break;
        const RoundMeta h{{meta.data(), k}}, d{{reinterpret_cast<uint64_t*>(g_fr.d_meta.p), k}};
        uint64_t slots = 0;
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t c = idx[j];
            h.in_off()[j] = in_off[c] + used[c];
            h.in_len()[j] = in_len[c] - used[c];
            h.out_cap()[j] = (cap[c] + 7) & ~7ull;
            h.out_off()[j] = slots;
            slots += h.out_cap()[j];
        }
        // round r - 2's frames left d_out[b] before it is reused (or reallocated)
        e = hipEventSynchronize(g_fr.ev_copied[b]);
        if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize(frames copy)");
        if ((st = g_fr.d_out[b].reserve(slots + 16, kFrameRounds))) return st;
        e = hipMemcpyAsync(d.p, h.p, h.inputs_bytes(), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(H2D round)");
        e = cpk::launch_read_message(g_fr.d_in.p, d.in_off(), d.in_len(), k, g_fr.d_out[b].p, d.out_off(), d.out_cap(),
                                     d.out_len(), d.consumed(), d.status(), s);
        if (e == hipSuccess) e = hipEventRecord(g_fr.ev_done[b], s);
        if (e != hipSuccess) return hip_fail(e, "read-message launch");
        e = hipMemcpyAsync(h.out_len(), d.out_len(), h.results_bytes(), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(D2H round)");
        // the round's frames go to `frames` as one copy of its slots up to the last good one
        uint64_t span = 0;
        uint32_t good = 0;
        for (uint32_t j = 0; j < k; ++j)
            if (h.status()[j] == CAPNP_PACKED_OK) {
                span = h.out_off()[j] + h.out_len()[j];
                ++good;
            }
        if (good) {
            if (fcur > frames_cap || span > frames_cap - fcur || good > max_frames - nf)
                return fail(CAPNP_PACKED_OUT_OF_SPACE, "frames buffer or frame table too small");
            // on the copy stream, while the next round decodes into the other buffer
            e = hipStreamWaitEvent(g_fr.copy, g_fr.ev_done[b], 0);
            if (e == hipSuccess)
                e = hipMemcpyAsync(frames + fcur, g_fr.d_out[b].p, span, hipMemcpyDeviceToHost, g_fr.copy);
            if (e == hipSuccess) e = hipEventRecord(g_fr.ev_copied[b], g_fr.copy);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(D2H frames)");
        }
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t c = idx[j];
            const int32_t rs = h.status()[j];
            const uint64_t len = h.out_len()[j];
            if (rs == CAPNP_PACKED_OK) {
                frame_off[nf] = fcur + h.out_off()[j];
                frame_len[nf] = len;
                frame_conn[nf] = c;
                ++nf;
                used[c] += h.consumed()[j];
                cap[c] = len < 8 ? 8 : len;
            } else if (rs == CAPNP_PACKED_OUT_OF_SPACE) {
                // the reader reported the framed length: next round, a slot that holds it
                cap[c] = std::max(2 * cap[c], len);
            } else {
                live[c] = 0;  // END_OF_STREAM: the rest waits for the next read; else the error
                status[c] = rs;
            }
        }
        fcur += (span + 7) & ~7ull;
    }
    for (uint32_t c = 0; c < n; ++c) {
        consumed[c] = used[c];
        slot_guess[c] = cap[c];
    }
    *n_frames = nf;
    return CAPNP_PACKED_OK;
}

}  // extern "C"


// ---------------------------------------------------------------------------
// Resumable framing of packed socket streams: Connection.handleRead
// (src/rpc/level2/connection.zig:153-203) with Framer state kept across reads
// (src/rpc/level0/framing.zig:42-90 keeps expected_total; reader.zig:84-156 is one pass).
// Each connection's unconsumed packed bytes live in a region of one device arena, so a read
// uploads only its new bytes (framer_layout.h has the regions). Per connection the session
// keeps the current message's framed length (need, from read_header_kernel once its header is
// decoded) and where its walk stopped (X: packed bytes from the message start, W: words
// decoded), so the next read's walk (frame_walk_kernel) starts there: a message split over k
// reads is uploaded once and walked once. A complete message is decoded straight from the
// arena into its frame slot (the batch decoder) and copied to the caller's frames buffer.
// ---------------------------------------------------------------------------
namespace {

// One capnp_packed_framer_read / _readv call: where its frames go, how far it has come, and
// the pass in hand.
struct FramerCall {
    uint8_t* frames;
    uint64_t frames_cap;
    uint64_t* frame_off;
    uint64_t* frame_len;
    uint32_t* frame_conn;
    uint32_t max_frames;
    int32_t* status;
    uint64_t fcur = 0;  // bytes of `frames` used
    uint32_t nf = 0;    // frames handed out
    bool full = false;  // the frames buffer or table ran out
    std::vector<uint8_t> dead, more;  // dead: an error this call (the connection was reset)
    std::vector<uint32_t> list;       // the pass's connections
    std::vector<uint64_t> adv;        // packed bytes of the pass's accepted messages, per connection
    std::vector<int32_t> perr;        // an error to report once the pass's frames are out
    std::vector<uint64_t> um;         // the pass's accepted messages: in_off, in_len, out_off, out_cap
    std::vector<uint32_t> uconn;      // and their connections
    uint64_t slots = 0;               // bytes of their frame slots
};

}  // namespace

struct capnp_packed_framer {
    std::mutex mu;
    uint32_t n = 0;
    hipStream_t s = nullptr;
    int dev = -1;  // the device the session was created on
    Buf<false> arena;
    framer_layout::Layout lay;         // per connection (host authoritative): its region and bytes
    std::vector<uint64_t> need, X, W;  // and the state of its current message
    Buf<false> d_state;   // StateBlock
    Buf<false> d_stage;   // a read's new bytes
    Buf<false> d_frames;  // a decode pass's frame slots
    Buf<false> d_spec;    // SpecBlock
    Buf<false> d_round;   // RoundBlock
    Buf<false> d_units;   // UnitBlock
    Buf<true> h_stage;    // page-locked gather of capnp_packed_framer_readv's reads
    // page-locked host sides of a read's metadata copies (no pageable staging per copy)
    Buf<true> pin_state, pin_tab, pin_units, pin_jobs;
    uint64_t uploaded = 0;                         // bytes copied H2D (new reads)
    uint64_t walk_passes = 0, table_windows = 0;   // walk passes run, windows they built tables for
    static constexpr uint32_t kWalkMessages = 64;  // messages a walk pass finds per connection
    // A read's upload and region copies need no synchronisation of their own: the walk pass's
    // synchronisation covers them. Until then d_stage and pin_jobs are theirs.
    bool jobs_inflight = false;

    ~capnp_packed_framer() {
        // the session's device is current for the teardown, whatever device the caller has
        // current now (the library's stream contexts are keyed by device and stream)
        int cur = -1;
        const bool switched = dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev &&
                              hipSetDevice(dev) == hipSuccess;
        if (s) {
            (void)hipStreamSynchronize(s);
            // the decode passes ran on s: drop the library's context of it (side stream, events,
            // class queue), or every session ever created would keep one
            (void)cpk::release_stream(s, dev);
        }
        for (Buf<false>* b : {&arena, &d_state, &d_stage, &d_frames, &d_spec, &d_round, &d_units}) b->release();
        for (Buf<true>* b : {&h_stage, &pin_state, &pin_tab, &pin_units, &pin_jobs}) b->release();
        if (s) (void)hipStreamDestroy(s);
        if (switched) (void)hipSetDevice(cur);
    }

    int settle() {  // the previous read's copies are done with d_stage and pin_jobs
        if (!jobs_inflight) return CAPNP_PACKED_OK;
        jobs_inflight = false;
        return launched(hipStreamSynchronize(s), "framer copy jobs");
    }

    // Run a plan's jobs into the arena `to`: as device jobs (dst, src, len) past the state
    // block's columns. The first `first` jobs run as a launch of their own, before the others
    // (stream order).
    int run_jobs(const framer_layout::Job* jobs, uint32_t nj, uint32_t first, uint8_t* to, bool wait) {
        if (nj == 0) return CAPNP_PACKED_OK;
        const uint64_t bytes = 3ull * nj * 8;
        int st = d_state.reserve(StateBlock::device_bytes(n, bytes), kSession);
        if (st) return st;
        uint64_t* const dj = StateBlock{d_state.p, n}.jobs();
        if ((st = pin_jobs.reserve(bytes, kSessionMeta))) return st;  // page-locked: no staged copy
        uint64_t* hj = reinterpret_cast<uint64_t*>(pin_jobs.p);
        for (uint32_t j = 0; j < nj; ++j, hj += 3) {
            const uint8_t* const from = jobs[j].src_kind == framer_layout::Src::kArena ? arena.p : d_stage.p;
            hj[0] = reinterpret_cast<uint64_t>(to + jobs[j].dst);
            hj[1] = reinterpret_cast<uint64_t>(from + jobs[j].src);
            hj[2] = jobs[j].len;
        }
        hipError_t e = hipMemcpyAsync(dj, pin_jobs.p, bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && first) e = cpk::launch_copy_jobs(dj, first, s);
        if (e == hipSuccess) e = cpk::launch_copy_jobs(dj + 3ull * first, nj - first, s);
        if (e == hipSuccess && wait) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "framer copy jobs");
        if (!wait) jobs_inflight = true;  // until the next synchronisation of s (a walk pass, or settle)
        return CAPNP_PACKED_OK;
    }

    int append(const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off, const uint64_t* in_len, bool staged);
    int walk_pass(const std::vector<uint32_t>& list);
    int decode_pass(FramerCall& C);
    void commit_pass(FramerCall& C);
};

// Step 1: the read's new bytes, one H2D into the staging buffer (staged: the caller already put
// them there on the session's stream), appended to the regions by the plan's copy jobs. The
// layout is committed only once every copy of the read is enqueued: a failed allocation or
// launch leaves the session as it was.
int capnp_packed_framer::append(const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off, const uint64_t* in_len,
                                bool staged) {
    int st = settle();
    if (st) return st;
    if (!in_bytes || !in_len) return CAPNP_PACKED_OK;
    if (!staged) {
        if ((st = d_stage.reserve(in_bytes + 32, kSession))) return st;
        const hipError_t e = hipMemcpyAsync(d_stage.p, in, in_bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(framer H2D)");
    }
    framer_layout::Plan P = framer_layout::plan_read(lay, in_off, in_len);
    const uint32_t nj = (uint32_t)P.jobs.size();
    if (P.rebuild) {
        struct NewArena : Buf<false> {  // freed unless committed; then the old arena is, in its place
            ~NewArena() { release(); }
        } na;
        if ((st = na.reserve(P.after.acap + 64, kSessionArena))) return st;
        // the moves run (and complete) now, from the current arena, which stays valid
        if ((st = run_jobs(P.jobs.data(), P.first, 0, na.p, true))) return st;
        if ((st = run_jobs(P.jobs.data() + P.first, nj - P.first, 0, na.p, false))) return st;
        std::swap(arena, static_cast<Buf<false>&>(na));
    } else if ((st = run_jobs(P.jobs.data(), nj, P.first, arena.p, false))) {
        return st;
    }
    lay = std::move(P.after);  // every copy of this read is enqueued: the regions describe the arena now
    uploaded += in_bytes;
    return CAPNP_PACKED_OK;
}

// Step 2: one walk over the held bytes of the listed connections, from where each one's last
// walk stopped. It leaves, page-locked on the host, the connections' need / X / W / status
// (pin_state, a StateBlock) and the messages found (pin_tab, RoundResults).
int capnp_packed_framer::walk_pass(const std::vector<uint32_t>& list) {
    const uint32_t k = (uint32_t)list.size();
    constexpr uint32_t M = kWalkMessages;
    const StateBlock h{pin_state.p, n}, d{d_state.p, n};
    for (uint32_t c = 0; c < n; ++c) {
        h.base()[c] = lay.off[c] + lay.m0[c];
        h.avail()[c] = lay.len[c] - lay.m0[c];
        h.need()[c] = need[c];
        h.X()[c] = X[c];
        h.W()[c] = W[c];
    }
    int st = d_round.reserve(RoundBlock::device_bytes(k, M), kSession);
    if (st) return st;
    const RoundBlock r{d_round.p, k, M};
    // window tables for the connections whose walk will cross whole windows inside one
    // message (crossed by lookups): the current message's framed bytes still to walk span
    // more than two windows, or, with its header not decoded yet, the held bytes span 64
    // windows. Many small messages end in nearly every window, where a table only costs.
    const uint64_t wb = cpk::framer_window_bytes(), wcap = cpk::framer_window_cap(k);
    std::vector<uint32_t> spec32(2ull * k, 0);  // first, count per listed connection
    std::vector<uint64_t> spec64(2ull * k, 0);  // their bytes: arena offset, length
    uint64_t T = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t c = list[j];
        const uint64_t span = lay.len[c] - lay.m0[c] - X[c];
        const uint64_t left = need[c] > 8 * W[c] ? need[c] - 8 * W[c] : 0;
        const bool lookups = need[c] ? left > 2 * wb : span > 64 * wb;
        uint64_t cnt = lookups && span > wb ? (span + wb - 1) / wb : 0;
        if (T + cnt > wcap) cnt = 0;
        spec32[j] = cnt ? (uint32_t)T : 0xFFFFFFFFu;
        spec32[k + j] = (uint32_t)cnt;
        spec64[j] = lay.off[c] + lay.m0[c] + X[c];
        spec64[k + j] = span;
        T += cnt;
    }
    SpecBlock sp(k, T);
    hipError_t e = hipSuccess;
    if (T) {
        if ((st = d_spec.reserve(sp.device_bytes(), kSession))) return st;
        sp.p = d_spec.p;
        e = hipMemcpyAsync(sp.windows(), &T, 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sp.first(), spec32.data(), 8ull * k, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sp.off(), spec64.data(), 16ull * k, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "framer window tables");
    }
    if ((st = pin_tab.reserve(RoundBlock::results_bytes(k, M), kSessionMeta))) return st;
    e = hipMemcpyAsync(d.base(), h.base(), h.inputs_bytes(), hipMemcpyHostToDevice, s);
    std::memcpy(h.list(), list.data(), 4ull * k);
    if (e == hipSuccess) e = hipMemcpyAsync(r.list(), h.list(), 4ull * k, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = cpk::launch_frame_walk(arena.p, r.list(), k, d.base(), d.avail(), d.need(), d.X(), d.W(), d.status(), M,
                                   r.counts(), r.table(), sp.queue(), T, sp.first(), sp.count(), sp.off(), sp.len(), s);
    if (e == hipSuccess) e = hipMemcpyAsync(h.need(), d.need(), h.results_bytes(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(pin_tab.p, r.counts(), RoundBlock::results_bytes(k, M), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "framer walk pass");
    jobs_inflight = false;
    ++walk_passes;
    table_windows += T;
    return CAPNP_PACKED_OK;
}

// Step 3: the whole messages the walk found, in order per connection, while the frames buffer
// and table hold them: decoded from the arena into frame slots, then to the caller's buffer.
int capnp_packed_framer::decode_pass(FramerCall& C) {
    const uint32_t k = (uint32_t)C.list.size();
    const StateBlock h{pin_state.p, n};
    const RoundResults found{reinterpret_cast<const uint32_t*>(pin_tab.p), k, kWalkMessages};
    C.um.clear();
    C.uconn.clear();
    C.slots = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t c = C.list[j];
        const uint32_t* const tj = found.messages(j);
        uint64_t at = 0;
        uint32_t m = 0;
        for (; m < found.count(j); ++m) {
            const uint64_t L = tj[2 * m + 1];
            if (C.nf + C.uconn.size() + 1 > C.max_frames || C.fcur + C.slots + L > C.frames_cap) {
                C.full = true;  // stays whole in its region: the next call pops it
                break;
            }
            C.um.insert(C.um.end(), {lay.off[c] + lay.m0[c] + at, tj[2 * m], C.slots, L});
            C.uconn.push_back(c);
            C.slots += (L + 7) & ~7ull;
            at += tj[2 * m];
        }
        C.adv[c] = at;
        C.perr[c] = CAPNP_PACKED_OK;
        C.more[c] = 0;
        if (m < found.count(j)) {  // the frames ran out: message m stays found whole (X at its end)
            h.need()[c] = tj[2 * m + 1];
            h.X()[c] = tj[2 * m];
            h.W()[c] = tj[2 * m + 1] / 8;
        } else if (h.status()[c] == CAPNP_PACKED_OK) {
            C.more[c] = 1;  // M messages: the next pass walks on from the last one's end
        } else if (h.status()[c] != CAPNP_PACKED_END_OF_STREAM) {
            C.perr[c] = h.status()[c];
        }
    }
    const uint32_t U = (uint32_t)C.uconn.size();
    if (!U) return CAPNP_PACKED_OK;
    int st;
    if ((st = d_frames.reserve(C.slots + 16, kSession))) return st;
    if ((st = d_units.reserve(UnitBlock::device_bytes(U), kSession))) return st;
    if ((st = pin_units.reserve(UnitBlock::host_bytes(U), kSessionMeta))) return st;
    const UnitBlock u{{reinterpret_cast<uint64_t*>(d_units.p), U}}, hu{{reinterpret_cast<uint64_t*>(pin_units.p), U}};
    for (uint32_t q = 0; q < U; ++q)
        for (uint32_t a = 0; a < 4; ++a) hu.col(a)[q] = C.um[4ull * q + a];
    hipError_t e = hipMemcpyAsync(u.p, hu.p, hu.inputs_bytes(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = cpk::launch_decode(arena.p, u.in_off(), u.in_len(), U, d_frames.p, u.out_off(), u.out_cap(), u.out_len(),
                               u.status(), true, nullptr, 0, s);
    if (e == hipSuccess) e = hipMemcpyAsync(C.frames + C.fcur, d_frames.p, C.slots, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hu.out_len(), u.out_len(), hu.results_bytes(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "framer decode pass");
    for (uint32_t q = 0; q < U; ++q) {
        if (hu.status()[q] != CAPNP_PACKED_OK || hu.out_len()[q] != hu.out_cap()[q])  // the walk verified the bytes
            return fail(CAPNP_PACKED_DEVICE_ERROR, "framer: a walked message did not decode to its framed length");
        C.frame_off[C.nf] = C.fcur + hu.out_off()[q];
        C.frame_len[C.nf] = hu.out_cap()[q];
        C.frame_conn[C.nf] = C.uconn[q];
        ++C.nf;
    }
    C.fcur += C.slots;
    return CAPNP_PACKED_OK;
}

// Step 4a: the pass's connections take their new state; an error is reported after the frames
// before it, and Connection.handleRead resets the framer on it (connection.zig:175-184).
void capnp_packed_framer::commit_pass(FramerCall& C) {
    const StateBlock h{pin_state.p, n};
    for (const uint32_t c : C.list) {
        lay.m0[c] += C.adv[c];
        need[c] = h.need()[c];
        X[c] = h.X()[c];
        W[c] = h.W()[c];
        if (C.perr[c] == CAPNP_PACKED_OK) continue;
        C.status[c] = C.perr[c];
        C.dead[c] = 1;
        lay.m0[c] = lay.len[c] = 0;
        need[c] = X[c] = W[c] = 0;
    }
}

namespace {

// capnp_packed_framer_read with f->mu held and its arguments checked: the new bytes, then passes
// (a walk over every connection's held messages, one decode of them) until no connection holds
// a whole message or the caller's frames are full.
int framer_read_locked(capnp_packed_framer* f, const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                       const uint64_t* in_len, bool staged, FramerCall& C, uint32_t* n_frames) {
    const uint32_t n = f->n;
    for (uint32_t c = 0; c < n; ++c) C.status[c] = CAPNP_PACKED_END_OF_STREAM;
    int st = f->append(in, in_bytes, in_off, in_len, staged);
    if (st) return st;
    if ((st = f->d_state.reserve(StateBlock::device_bytes(n, 0), kSession))) return st;  // see StateBlock
    if ((st = f->pin_state.reserve(StateBlock::host_bytes(n), kSessionMeta))) return st;
    C.dead.assign(n, 0);
    C.more.resize(n);
    C.adv.resize(n);
    C.perr.resize(n);
    for (uint32_t c = 0; c < n; ++c) C.more[c] = f->lay.len[c] > f->lay.m0[c];
    while (!C.full) {
        C.list.clear();
        for (uint32_t c = 0; c < n; ++c)
            if (!C.dead[c] && C.more[c]) C.list.push_back(c);
        if (C.list.empty()) break;
        if ((st = f->walk_pass(C.list))) return st;
        if ((st = f->decode_pass(C))) return st;
        f->commit_pass(C);
    }
    *n_frames = C.nf;
    if ((st = f->settle())) return st;  // no pass ran after the upload: the caller's bytes are consumed
    return C.full ? fail(CAPNP_PACKED_OUT_OF_SPACE, "frames buffer or frame table full: call again to pop the rest")
                  : CAPNP_PACKED_OK;
}

int framer_check(capnp_packed_framer* f, uint32_t conn) {
    if (!f) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "framer is null");
    if (conn >= f->n) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "connection index out of range");
    return CAPNP_PACKED_OK;
}

// The gather of capnp_packed_framer_readv: bytes [r0, r1) of the connections' reads, laid end
// to end at their prefix offsets, into the session's page-locked staging, by byte range over up
// to 8 threads from 4 MiB up.
void gather_reads(uint8_t* dst, const uint8_t* const* ptr, const uint64_t* len, const uint64_t* off, uint32_t n,
                  uint64_t r0, uint64_t r1) {
    auto copy_range = [=](uint64_t b0, uint64_t b1) {
        // the first connection whose bytes end past b0
        uint32_t c = (uint32_t)(std::upper_bound(off, off + n, b0) - off);
        c = c ? c - 1 : 0;
        for (; c < n && off[c] < b1; ++c) {
            if (!len[c]) continue;
            const uint64_t lo = std::max(off[c], b0), hi = std::min(off[c] + len[c], b1);
            if (lo < hi) std::memcpy(dst + lo, ptr[c] + (lo - off[c]), hi - lo);
        }
    };
    const uint64_t total = r1 - r0;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned T = total < (4ull << 20) ? 1u : std::max(1u, std::min(8u, hw ? hw : 1u));
    std::vector<std::thread> th;
    try {
        for (unsigned t = 1; t < T; ++t) th.emplace_back(copy_range, r0 + total * t / T, r0 + total * (t + 1) / T);
    } catch (...) {  // no threads: the rest on this one
        copy_range(r0 + total * (th.size() + 1) / T, r1);
    }
    copy_range(r0, r0 + total / T);
    for (auto& x : th) x.join();
}

int framer_args(capnp_packed_framer* f, uint8_t* frames, uint64_t frames_cap, uint64_t* frame_off,
                uint64_t* frame_len, uint32_t* frame_conn, uint32_t max_frames, int32_t* status, uint32_t* n_frames) {
    if (!n_frames) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "n_frames is null");
    *n_frames = 0;
    if (!f) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "framer is null");
    if (!status || (max_frames && (!frame_off || !frame_len || !frame_conn)) || (frames_cap && !frames))
        return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    return CAPNP_PACKED_OK;
}

}  // namespace

extern "C" {

int capnp_packed_framer_create(uint32_t n_conns, capnp_packed_framer** out) {
    if (!out) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (n_conns == 0) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "a framer needs at least one connection");
    int st = ensure_device();
    if (st) return st;
    capnp_packed_framer* f = new (std::nothrow) capnp_packed_framer();
    if (!f) return fail(CAPNP_PACKED_OUT_OF_SPACE, "framer allocation");
    f->n = n_conns;
    if (hipGetDevice(&f->dev) != hipSuccess) f->dev = -1;
    for (auto* v : {&f->lay.off, &f->lay.cap, &f->lay.m0, &f->lay.len, &f->need, &f->X, &f->W}) v->assign(n_conns, 0);
    hipError_t e = hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking);
    if (e != hipSuccess) {
        f->s = nullptr;
        delete f;
        return hip_fail(e, "hipStreamCreate(framer session)");
    }
    *out = f;
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_destroy(capnp_packed_framer* f) {
    if (!f) return CAPNP_PACKED_OK;
    delete f;  // synchronises its stream first
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_reset(capnp_packed_framer* f, uint32_t conn) {
    int st = framer_check(f, conn);
    if (st) return st;
    std::lock_guard<std::mutex> lock(f->mu);
    f->lay.m0[conn] = f->lay.len[conn] = 0;
    f->need[conn] = f->X[conn] = f->W[conn] = 0;
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_buffered(capnp_packed_framer* f, uint32_t conn, uint64_t* bytes) {
    int st = framer_check(f, conn);
    if (st) return st;
    if (!bytes) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "bytes is null");
    std::lock_guard<std::mutex> lock(f->mu);
    *bytes = f->lay.len[conn] - f->lay.m0[conn];
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_expected(capnp_packed_framer* f, uint32_t conn, uint64_t* framed_bytes) {
    int st = framer_check(f, conn);
    if (st) return st;
    if (!framed_bytes) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "framed_bytes is null");
    std::lock_guard<std::mutex> lock(f->mu);
    *framed_bytes = f->need[conn];
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_stats(capnp_packed_framer* f, uint64_t* uploaded, uint64_t* moved) {
    if (!f || !uploaded || !moved) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    std::lock_guard<std::mutex> lock(f->mu);
    *uploaded = f->uploaded;
    *moved = f->lay.moved;
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_walk_stats(capnp_packed_framer* f, uint64_t* passes, uint64_t* table_windows) {
    if (!f || !passes || !table_windows) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    std::lock_guard<std::mutex> lock(f->mu);
    *passes = f->walk_passes;
    *table_windows = f->table_windows;
    return CAPNP_PACKED_OK;
}

int capnp_packed_framer_read(capnp_packed_framer* f, const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                             const uint64_t* in_len, uint8_t* frames, uint64_t frames_cap, uint64_t* frame_off,
                             uint64_t* frame_len, uint32_t* frame_conn, uint32_t max_frames, int32_t* status,
                             uint32_t* n_frames) {
    int st = framer_args(f, frames, frames_cap, frame_off, frame_len, frame_conn, max_frames, status, n_frames);
    if (st) return st;
    const uint32_t n = f->n;
    if (in_bytes && (!in || !in_off || !in_len)) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    if (in_len)
        for (uint32_t c = 0; c < n; ++c)
            if (in_len[c] && (!in_off || in_off[c] > in_bytes || in_len[c] > in_bytes - in_off[c]))
                return fail(CAPNP_PACKED_INVALID_ARGUMENT, "connection bytes outside the input buffer");
    std::lock_guard<std::mutex> lock(f->mu);
    FramerCall C{frames, frames_cap, frame_off, frame_len, frame_conn, max_frames, status};
    return framer_read_locked(f, in, in_bytes, in_off, in_len, false, C, n_frames);
}

int capnp_packed_framer_readv(capnp_packed_framer* f, const uint8_t* const* in_ptr, const uint64_t* in_len,
                              uint8_t* frames, uint64_t frames_cap, uint64_t* frame_off, uint64_t* frame_len,
                              uint32_t* frame_conn, uint32_t max_frames, int32_t* status, uint32_t* n_frames) {
    int st = framer_args(f, frames, frames_cap, frame_off, frame_len, frame_conn, max_frames, status, n_frames);
    if (st) return st;
    const uint32_t n = f->n;
    if (!in_ptr || !in_len) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "null pointer");
    std::vector<uint64_t> off(n);
    uint64_t total = 0;
    for (uint32_t c = 0; c < n; ++c) {
        if (in_len[c] && !in_ptr[c]) return fail(CAPNP_PACKED_INVALID_ARGUMENT, "a connection's bytes are null");
        off[c] = total;
        total += in_len[c];
    }
    std::lock_guard<std::mutex> lock(f->mu);
    if (total) {
        // the previous call's upload from the staging has finished (each call ends synchronised)
        if ((st = f->h_stage.reserve(total, kSessionStaging))) return st;
        // gather and upload in 32-MiB pieces: piece i's H2D runs while piece i + 1 is gathered
        if ((st = f->settle())) return st;  // the previous read's copies are done with d_stage
        if ((st = f->d_stage.reserve(total + 32, kSession))) return st;
        constexpr uint64_t kPiece = 32ull << 20;
        for (uint64_t r0 = 0; r0 < total; r0 += kPiece) {
            const uint64_t r1 = std::min(total, r0 + kPiece);
            gather_reads(f->h_stage.p, in_ptr, in_len, off.data(), n, r0, r1);
            const hipError_t e =
                hipMemcpyAsync(f->d_stage.p + r0, f->h_stage.p + r0, r1 - r0, hipMemcpyHostToDevice, f->s);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(framer H2D)");
        }
    }
    FramerCall C{frames, frames_cap, frame_off, frame_len, frame_conn, max_frames, status};
    return framer_read_locked(f, total ? f->h_stage.p : nullptr, total, total ? off.data() : nullptr,
                              total ? in_len : nullptr, true, C, n_frames);
}

}  // extern "C"
