// kernels/side_launch.h
// Host only: the per-(device, caller stream) side-launch context (StreamCtx, SideLaunch: side
// streams, fork / join events, the library's class workspace), the process-wide launch policy
// flags, and the kernels.h calls that manage the contexts (queue_bytes, set_launch_flags,
// release_stream, stream_queue_info, stream_context_count). DESIGN.md §2.6 (`SideLaunch`).
// No kernel needs it and it needs no kernel; its statics belong to the one translation unit
// that includes it, packed_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "capnp_packed.h"
#include "class_ws.h"
#include "kernels.h"

namespace cpk {

// Side stream for the long-unit kernels (encode_tiled_kernel, the decode fallback).
// They select their units by a test on the unit's own lengths, so they need nothing
// from the main kernels and run beside them: a batch whose few long units would
// otherwise run alone after the main grid (config C5's tail) overlaps them with it.
// fork(): the side stream waits for everything already on the caller's stream;
// join(): the caller's stream waits for the side stream's kernels.
//
// Every (device, caller stream) pair has its own context: side stream, fork/join
// events and long-unit queue, so batches on independent caller streams never wait
// on each other, and a graph captured from one stream shares nothing with eager
// work on another. The context's mutex keeps one caller's record/wait pairs and
// queue reset together. A queue that has to grow is replaced by one of at least twice its
// size (so a stream sees O(log n) replacements): the old one is freed after the stream
// drains, unless a hipGraph capture used it (a captured graph may still reference it; it is
// then kept until capnp_packed_stream_release). Growing is refused during a capture.
// Callers that pass their own workspace (capnp_packed_*_batch_ws) use it as the
// queue instead, so nothing of the library's is baked into their graphs.
struct StreamCtx {
    std::mutex mu;
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    hipStream_t s2 = nullptr;  // a second side stream (CAPNP_PACKED_LAUNCH_MID_SIDE_STREAM: C5's mid units)
    hipEvent_t join2 = nullptr;
    uint32_t* q = nullptr;  // class workspace (queue_bytes; class_ws.h)
    uint64_t qcap = 0;
    bool q_captured = false;         // q was used inside a hipGraph capture
    std::vector<uint32_t*> retired;  // replaced queues a capture used (graphs may reference them)
    ~StreamCtx() {
        for (uint32_t* r : retired) (void)hipFree(r);
        if (q) (void)hipFree(q);
        if (s) (void)hipStreamDestroy(s);
        if (s2) (void)hipStreamDestroy(s2);
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        if (join2) (void)hipEventDestroy(join2);
    }
};
static std::mutex g_ctx_mu;
// shared_ptr: a batch being enqueued keeps its context alive even if capnp_packed_stream_release
// drops it from the map meanwhile (no use-after-free, whatever the callers do).
static std::map<std::pair<int, uintptr_t>, std::shared_ptr<StreamCtx>> g_ctx;

size_t queue_bytes(uint32_t n) { return class_ws_bytes(n); }

// Launch policy (capnp_packed_set_launch_flags, process-wide; no result depends on it):
//   CAPNP_PACKED_LAUNCH_LONG_INLINE      the long-unit kernels run after the main grid on the
//                                        caller's stream instead of on a side stream;
//   CAPNP_PACKED_LAUNCH_MID_SIDE_STREAM  decode: a batch's mid units on a second side stream,
//                                        launched before the small units' kernel, whose grid then
//                                        takes 85% of its resident size. Round 3:
//                                        C5 decode 0.678 -> 0.660 ms, but the headline (all mid
//                                        units) 2.474 -> 2.499 ms from the extra fork and join.
//   CAPNP_PACKED_LAUNCH_CLASS_SCAN       the class pass's scan as its own kernel (class_scan_kernel)
//                                        also for batches of at most 1M units, whose scatter
//                                        otherwise does it (the path larger batches always take).
static std::atomic<uint32_t> g_launch_flags{0};
uint32_t set_launch_flags(uint32_t f) { return g_launch_flags.exchange(f); }

class SideLaunch {
  public:
    SideLaunch(hipStream_t main, void* ws, size_t ws_bytes) : main_(main), ws_(ws), ws_bytes_(ws_bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return;
        {
            std::lock_guard<std::mutex> g(g_ctx_mu);
            std::shared_ptr<StreamCtx>& c = g_ctx[{dev, reinterpret_cast<uintptr_t>(main)}];
            if (!c) c = std::make_shared<StreamCtx>();
            ctx_ = c;
        }
        lock_ = std::unique_lock<std::mutex>(ctx_->mu);
        if (g_launch_flags.load(std::memory_order_relaxed) & CAPNP_PACKED_LAUNCH_LONG_INLINE) {
            side_ = main_;
            ok_ = true;
            return;
        }
        if (!ctx_->s) {
            if (hipStreamCreateWithFlags(&ctx_->s, hipStreamNonBlocking) != hipSuccess) {
                ctx_->s = nullptr;
                return;
            }
            if (hipEventCreateWithFlags(&ctx_->fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ctx_->join, hipEventDisableTiming) != hipSuccess) {
                (void)hipStreamDestroy(ctx_->s);
                ctx_->s = nullptr;
                return;
            }
        }
        side_ = ctx_->s;
        ok_ = true;
    }
    // the stream the long-unit kernels go on (after fork())
    hipStream_t stream() const { return side_; }
    // The side stream waits for everything enqueued on the caller's stream so far.
    hipError_t fork() {
        if (!ok_ || side_ == main_ || forked_) return ok_ ? hipSuccess : hipErrorNotReady;
        hipError_t e = hipEventRecord(ctx_->fork, main_);
        if (e == hipSuccess) e = hipStreamWaitEvent(side_, ctx_->fork, 0);
        if (e == hipSuccess) forked_ = true;
        return e;
    }
    // The class workspace for a batch of n units (queue_bytes); launch_classes must run on it
    // next (class_scan_kernel clears its counters); nullptr when the side stream or the queue
    // cannot be set up.
    uint32_t* queue(uint32_t n) {
        if (!ok_) return nullptr;
        uint32_t* q = nullptr;
        if (ws_) {
            if (ws_bytes_ < queue_bytes(n)) return nullptr;
            q = static_cast<uint32_t*>(ws_);
        } else {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(main_, &cs) != hipSuccess) return nullptr;
            const bool capturing = cs != hipStreamCaptureStatusNone;
            if (ctx_->qcap < n) {
                if (capturing) return nullptr;
                uint64_t cap = 2 * ctx_->qcap;
                cap = cap < n ? n : cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap;
                uint32_t* nq = nullptr;
                if (hipMalloc(reinterpret_cast<void**>(&nq), queue_bytes((uint32_t)cap)) != hipSuccess) return nullptr;
                if (ctx_->q) {
                    if (ctx_->q_captured) {
                        ctx_->retired.push_back(ctx_->q);
                    } else {  // only this stream's batches used it (the side stream joins back)
                        if (hipStreamSynchronize(main_) != hipSuccess) {
                            (void)hipFree(nq);
                            return nullptr;
                        }
                        (void)hipFree(ctx_->q);
                    }
                }
                ctx_->q = nq;
                ctx_->qcap = cap;
                ctx_->q_captured = false;
            }
            ctx_->q_captured |= capturing;
            q = ctx_->q;
        }
        return q;  // its head (counters, cursors) is cleared by class_scan_kernel
    }
    // A second side stream, forked like the first (after fork()); the caller's stream when it
    // cannot be set up.
    hipStream_t stream2() {
        if (!forked_) return main_;
        if (forked2_) return ctx_->s2;
        if (!ctx_->s2) {
            if (hipStreamCreateWithFlags(&ctx_->s2, hipStreamNonBlocking) != hipSuccess) {
                ctx_->s2 = nullptr;
                return main_;
            }
            if (hipEventCreateWithFlags(&ctx_->join2, hipEventDisableTiming) != hipSuccess) {
                (void)hipStreamDestroy(ctx_->s2);
                ctx_->s2 = nullptr;
                return main_;
            }
        }
        if (hipStreamWaitEvent(ctx_->s2, ctx_->fork, 0) != hipSuccess) return main_;
        forked2_ = true;
        return ctx_->s2;
    }
    hipError_t join() {
        if (!forked_) return hipSuccess;
        forked_ = false;
        hipError_t e = hipEventRecord(ctx_->join, side_);
        if (e == hipSuccess) e = hipStreamWaitEvent(main_, ctx_->join, 0);
        if (forked2_) {
            forked2_ = false;
            hipError_t e2 = hipEventRecord(ctx_->join2, ctx_->s2);
            if (e2 == hipSuccess) e2 = hipStreamWaitEvent(main_, ctx_->join2, 0);
            if (e == hipSuccess) e = e2;
        }
        return e;
    }
    ~SideLaunch() { (void)join(); }

  private:
    hipStream_t main_;
    void* ws_;
    size_t ws_bytes_;
    std::shared_ptr<StreamCtx> ctx_;  // held until after the join and the unlock
    std::unique_lock<std::mutex> lock_;
    hipStream_t side_ = nullptr;
    bool ok_ = false, forked_ = false, forked2_ = false;
};

// Drop the library's context of a caller stream (its side stream, events and queues, also
// those captured graphs used): after the stream's work is done and before it is destroyed.
hipError_t release_stream(hipStream_t stream, int dev) {
    hipError_t e = hipSuccess;
    if (dev < 0) e = hipGetDevice(&dev);  // contexts are keyed by (device, stream)
    if (e != hipSuccess) return e;
    std::shared_ptr<StreamCtx> c;
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        auto it = g_ctx.find({dev, reinterpret_cast<uintptr_t>(stream)});
        if (it == g_ctx.end()) return hipSuccess;
        c = std::move(it->second);
        g_ctx.erase(it);
    }
    std::lock_guard<std::mutex> g(c->mu);  // no batch of this stream is being enqueued
    e = hipStreamSynchronize(stream);
    if (e == hipSuccess && c->s) e = hipStreamSynchronize(c->s);
    return e;  // ~StreamCtx frees the rest
}

// The per-stream queue the library holds for `stream`: its bytes, and how many replaced
// queues it keeps because a capture used them (tests: growth stays bounded).
void stream_queue_info(hipStream_t stream, size_t* bytes, uint32_t* kept) {
    *bytes = 0;
    *kept = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> g(g_ctx_mu);
    auto it = g_ctx.find({dev, reinterpret_cast<uintptr_t>(stream)});
    if (it == g_ctx.end()) return;
    std::lock_guard<std::mutex> g2(it->second->mu);
    *bytes = it->second->q ? queue_bytes((uint32_t)it->second->qcap) : 0;
    *kept = (uint32_t)it->second->retired.size();
}

uint32_t stream_context_count() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> g(g_ctx_mu);
    uint32_t k = 0;
    for (const auto& kv : g_ctx) k += kv.first.first == dev;
    return k;
}

}  // namespace cpk
