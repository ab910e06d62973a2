// owners.hpp -- the ONE place where the host side of the C ABI allocates and frees device memory and pinned host memory and
// creates and destroys streams and events.  Everything a handle object (pg_engine, pg_composer, pg_comm, pg_gather_pipeline,
// pg_g2_prepared) or a call keeps is a member of one of these types and is released by its destructor.
//
// THE RULE: a destructor here neither selects a device nor waits for work.  The pg_*_destroy function (or the call) that lets an
// owner go does both first -- its device current, its streams drained -- and then only deletes.
//
// Included by host_util.hpp.  Needs <hip/hip_runtime.h>, the C header and host_util.hpp's Carve, no device code: a plain host
// compiler builds it against a stand-in runtime (tests/cpp/owners_host.cpp, g++, also under ASan + UBSan).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/plonk_gadgets_hip.h"
#include "composer_cols.hpp"
#include "host_util.hpp"  // Carve (this file is included from its second part: the first is complete by then)

namespace {

using pg::Carve;

thread_local std::string g_last_error;

pg_status fail(pg_status s, const std::string &msg) {
    g_last_error = msg;
    return s;
}

#define PG_HIP_TRY(expr)                                                                \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(PG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define PG_TRY(expr)                   \
    do {                               \
        pg_status _s = (expr);         \
        if (_s != PG_OK) return _s;    \
    } while (0)

struct DeviceMem {
    static constexpr const char *what = "hipMalloc(&p_, bytes)";
    static hipError_t allocate(void **p, uint64_t bytes) { return hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static constexpr const char *what = "hipHostMalloc(&p_, bytes, hipHostMallocDefault)";
    static hipError_t allocate(void **p, uint64_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void *p) { (void)hipHostFree(p); }
};

// A grow-only buffer that owns its memory.  reserve() allocates on the CURRENT device and neither synchronises nor clears: a
// caller whose buffer may still be read by work in flight orders that itself (hipFree waits for the device).  Movable: "allocate
// the new one, fill it, then let the old one go" is a reserve() into a fresh buffer and a move assignment once that succeeded.
template <class Mem>
class Buffer {
  public:
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(bytes_, o.bytes_);
        }
        return *this;
    }
    ~Buffer() { reset(); }
    void reset() {
        if (p_) Mem::release(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // at least `bytes`; what the buffer held is lost when it grows, and a failed allocation leaves it empty
    pg_status reserve(uint64_t bytes) {
        if (bytes <= bytes_) return PG_OK;
        reset();
        const hipError_t err = Mem::allocate(&p_, bytes);
        if (err != hipSuccess) {
            p_ = nullptr;
            return fail(PG_ERR_HIP, std::string(Mem::what) + ": " + hipGetErrorString(err));
        }
        bytes_ = bytes;
        return PG_OK;
    }
    // reserve what `layout` measures, then let it place its parts: layout(Carve) names the parts and returns Carve::bytes()
    template <class Layout>
    pg_status carve(uint64_t align, Layout &&layout) {
        PG_TRY(reserve(layout(Carve(align))));
        layout(Carve(align, p_));
        return PG_OK;
    }
    void *get() const { return p_; }
    uint64_t size() const { return bytes_; }
    template <typename T>
    T *as() const { return static_cast<T *>(p_); }

  private:
    void *p_ = nullptr;
    uint64_t bytes_ = 0;
};
using Scratch = Buffer<DeviceMem>;  // device memory
using Pinned = Buffer<PinnedMem>;   // page-locked host memory

// An event, made by create(flags) on the current device.
class Event {
  public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    pg_status create(unsigned flags) {
        if (!ev_) PG_HIP_TRY(hipEventCreateWithFlags(&ev_, flags));
        return PG_OK;
    }
    hipEvent_t get() const { return ev_; }

  private:
    hipEvent_t ev_ = nullptr;
};

// A stream, made by one of the two create calls on the current device.  The destructor does not wait for it.
class Stream {
  public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (st_) (void)hipStreamDestroy(st_);
    }
    pg_status create(unsigned flags) {
        PG_HIP_TRY(hipStreamCreateWithFlags(&st_, flags));
        return PG_OK;
    }
    pg_status create_with_priority(unsigned flags, int priority) {
        PG_HIP_TRY(hipStreamCreateWithPriority(&st_, flags, priority));
        return PG_OK;
    }
    hipStream_t get() const { return st_; }

  private:
    hipStream_t st_ = nullptr;
};

// Pinned memory that the host fills and an asynchronous copy reads, reused only after the copy that last read it has left:
// acquire() waits for the event that sent() recorded behind that copy.  With a device twin of the same size where the copy's
// destination lives as long as its source.  The event is made by the first acquire().
class Staging {
  public:
    // the buffers may be rewritten and hold at least `bytes` each (grow-only; what they held is lost when they grow)
    pg_status acquire(uint64_t bytes, bool with_twin) {
        PG_TRY(ev_.create(hipEventDisableTiming));
        PG_TRY(wait());
        if (bytes <= size_) return PG_OK;
        size_ = 0;  // (a twin that fails to grow leaves the pair at 0: the next acquire allocates it again)
        PG_TRY(h_.reserve(bytes));
        if (with_twin) PG_TRY(d_.reserve(bytes));
        size_ = bytes;
        return PG_OK;
    }
    // everything enqueued on `st` so far has to leave before the next acquire() returns
    // (the runtime's own status: the callers word the failure)
    hipError_t sent(hipStream_t st) {
        const hipError_t err = hipEventRecord(ev_.get(), st);
        if (err == hipSuccess) pending_ = true;
        return err;
    }
    pg_status wait() {
        if (pending_) PG_HIP_TRY(hipEventSynchronize(ev_.get()));
        pending_ = false;
        return PG_OK;
    }
    char *host() const { return h_.as<char>(); }
    char *device() const { return d_.as<char>(); }
    uint64_t size() const { return size_; }

  private:
    Pinned h_;
    Scratch d_;
    uint64_t size_ = 0;
    Event ev_;
    bool pending_ = false;
};

// Device buffers that live for one call: handed out one by one and released on every way out of the call -- after the stream
// has drained, for work may still read them.
class CallBuffers {
  public:
    explicit CallBuffers(hipStream_t st) : stream_(st) {}
    ~CallBuffers() {
        if (!held_.empty()) (void)hipStreamSynchronize(stream_);
    }
    template <typename T>
    pg_status take(T **out, uint64_t bytes) {
        Scratch s;
        PG_TRY(s.reserve(bytes));
        *out = s.as<T>();
        held_.push_back(std::move(s));
        return PG_OK;
    }

  private:
    hipStream_t stream_;
    std::vector<Scratch> held_;
};

// The composer's nine columns (five selectors of 32 bytes a row, three wires of 8, the Variables' values of 32 each) in one of
// two layouts: nine allocations (stride 0), or ONE block laid out by pg_columns_slab_layout with the selector columns `stride`
// bytes apart.  create() and grow() build the new arrays in a store of their own and take them over only when everything has
// succeeded: on any failure they return, the new arrays free themselves, and this store is what it was.
class ColumnStore {
  public:
    const pg::ComposerCols &view() const { return v_; }
    uint64_t gate_cap() const { return gate_cap_; }
    uint64_t var_cap() const { return var_cap_; }
    uint64_t stride() const { return stride_; }

    // nine separate arrays for an empty store
    pg_status create(uint64_t gate_cap, uint64_t var_cap) {
        ColumnStore fresh;
        PG_TRY(fresh.allocate(gate_cap, var_cap, 0, true, true));
        adopt(fresh, gate_cap, var_cap, 0);
        return PG_OK;
    }

    // New arrays of (at least) these capacities in the layout `stride` asks for; the live part -- live_rows rows, live_vars
    // Variables -- is copied on `st`, and the old arrays are released once that copy is done.  Separate arrays: only those whose
    // capacity grows move.  One block, or another layout than before: all nine move, and the old ones and the new ones are
    // alive together until the copy is done.
    pg_status grow(uint64_t gate_cap, uint64_t var_cap, uint64_t stride, uint64_t live_rows, uint64_t live_vars, hipStream_t st) {
        if (gate_cap < gate_cap_) gate_cap = gate_cap_;
        if (var_cap < var_cap_) var_cap = var_cap_;
        const bool all = stride != stride_ || stride != 0;
        const bool move_rows = all || gate_cap > gate_cap_, move_vars = all || var_cap > var_cap_;
        if (!move_rows && !move_vars) return PG_OK;
        ColumnStore fresh;
        PG_TRY(fresh.allocate(gate_cap, var_cap, stride, move_rows, move_vars));
        hipError_t err = hipSuccess;
        for (int i = 0; i < 9; i++) {
            const uint64_t bytes = i < 5 ? live_rows * 32 : i < 8 ? live_rows * 8 : live_vars * 32;
            if (err == hipSuccess && bytes && fresh.col(i))
                err = hipMemcpyAsync(fresh.col(i), col(i), bytes, hipMemcpyDeviceToDevice, st);
        }
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) {  // this store keeps its arrays; the new ones go once nothing writes to them any more
            (void)hipStreamSynchronize(st);
            return fail(PG_ERR_HIP, std::string("growing the composer: ") + hipGetErrorString(err));
        }
        adopt(fresh, gate_cap, var_cap, stride);
        return PG_OK;
    }

  private:
    // column i of the view: q_m, q_l, q_r, q_o, q_c, w_l, w_r, w_o, the Variables
    void *col(int i) const { return i < 5 ? (void *)v_.q[i] : i < 8 ? (void *)v_.w[i - 5] : (void *)v_.vars; }
    void set_col(int i, void *p) {
        if (i < 5) v_.q[i] = static_cast<uint4 *>(p);
        else if (i < 8) v_.w[i - 5] = static_cast<uint64_t *>(p);
        else v_.vars = static_cast<uint4 *>(p);
    }
    // into an empty store: the block, or the row arrays and / or the Variables' array
    pg_status allocate(uint64_t gate_cap, uint64_t var_cap, uint64_t stride, bool rows, bool vars) {
        pg_status st = PG_OK;
        if (stride) {
            uint64_t off[9], total = 0;
            PG_TRY(pg_columns_slab_layout(gate_cap, var_cap, stride, off, &total));
            // said before the allocation is tried, with the figures, rather than as a bare out-of-memory afterwards
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total > free_b)
                return fail(PG_ERR_CAPACITY, "composer with spread columns cannot grow to " + std::to_string(gate_cap) + " rows / " +
                                                 std::to_string(var_cap) + " variables: the new block of " + std::to_string(total >> 20) +
                                                 " MiB (selector columns " + std::to_string(stride >> 20) +
                                                 " MiB apart) must exist beside the old one during the move, and " +
                                                 std::to_string(free_b >> 20) + " MiB of device memory are free; reserve the final "
                                                 "capacity before pg_composer_spread_columns, or use a smaller stride");
            st = mem_[0].reserve(total);
            for (int i = 0; i < 9 && st == PG_OK; i++) set_col(i, mem_[0].as<char>() + off[i]);
        } else {
            for (int i = 0; i < 9 && st == PG_OK; i++) {
                if (!(i < 8 ? rows : vars)) continue;
                st = mem_[i].reserve(i < 5 ? gate_cap * 32 : i < 8 ? gate_cap * 8 : var_cap * 32);
                set_col(i, mem_[i].get());
            }
        }
        if (st == PG_OK) return PG_OK;
        (void)hipGetLastError();  // the refused allocation's error is not left behind for the next launch to find
        return fail(PG_ERR_CAPACITY, "composer cannot grow to " + std::to_string(gate_cap) + " rows / " + std::to_string(var_cap) +
                                         " variables: out of device memory");
    }
    // take over the arrays `fresh` holds (the old ones are released); where the layout changes or is one block, that is all of them
    void adopt(ColumnStore &fresh, uint64_t gate_cap, uint64_t var_cap, uint64_t stride) {
        const bool all = stride != stride_ || stride != 0;
        for (int i = 0; i < 9; i++) {
            if (!all && !fresh.col(i)) continue;
            mem_[i] = std::move(fresh.mem_[i]);
            set_col(i, fresh.col(i));
        }
        gate_cap_ = gate_cap, var_cap_ = var_cap, stride_ = stride;
    }

    Scratch mem_[9];  // separate arrays: one each, in col()'s order; one block: mem_[0] alone
    pg::ComposerCols v_{};
    uint64_t gate_cap_ = 0, var_cap_ = 0, stride_ = 0;
};

}  // namespace
