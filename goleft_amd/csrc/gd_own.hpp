// gd_own.hpp -- the four owners of what the device ABI takes from the HIP runtime: a typed device array, a typed
// page-locked host array, an event and a stream.  Each is move-only, gives back what it owns when it goes, and can hold
// something it does not own (a caller's records, a caller's stream), which it never gives back.  Nothing here knows a
// gd_ctx: the functions return hipError_t, and the header needs only the runtime's declarations (it is tested on the
// host alone, against stand-ins for the hip* functions: tests/emul/own_asan_main.cpp).  hipFree and hipHostFree wait for
// the whole device, so nothing frees behind the caller's back but a destructor and a move-assignment onto a full owner:
// alloc() and create() on a full owner are refused.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace gd_own __attribute__((visibility("hidden"))) {       // (a library that includes this exports none of it)

struct DeviceMem {
    static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t put(void* p) { return hipFree(p); }
};

struct PinnedMem {
    static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t put(void* p) { return hipHostFree(p); }
};

// Pointer and capacity (in elements) of one block, together.
template <typename T, class Mem>
class Arr {
    T* p_ = nullptr;
    size_t cap_ = 0;
    bool owned_ = true;

public:
    Arr() = default;
    Arr(const Arr&) = delete;
    Arr& operator=(const Arr&) = delete;
    Arr(Arr&& o) noexcept : p_(o.p_), cap_(o.cap_), owned_(o.owned_) { o.forget(); }
    Arr& operator=(Arr&& o) noexcept                     // (frees what this one owned)
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; owned_ = o.owned_; o.forget(); }
        return *this;
    }
    ~Arr() { reset(); }

    // Room for `count` elements (0: one) in an EMPTY owner; a failure leaves it empty.
    hipError_t alloc(size_t count)
    {
        if (p_) return hipErrorInvalidValue;
        if (count == 0) count = 1;
        void* q = nullptr;
        const hipError_t e = Mem::get(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(q); cap_ = count; owned_ = true;
        return hipSuccess;
    }
    // Empty afterwards whatever the runtime answers: reset() ignores the answer as a destructor has to.
    hipError_t reset_checked()
    {
        const hipError_t e = p_ && owned_ ? Mem::put(p_) : hipSuccess;
        forget();
        return e;
    }
    void reset() { (void)reset_checked(); }
    // The block is the caller's from here on.
    T* release() { T* q = p_; forget(); return q; }
    // A block somebody else frees (this owner's own block, if any, goes first).
    void borrow(T* p, size_t count) { reset(); p_ = p; cap_ = p ? count : 0; owned_ = false; }

    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    template <typename U> U* as() const { return reinterpret_cast<U*>(p_); }

private:
    void forget() { p_ = nullptr; cap_ = 0; owned_ = true; }
};

template <typename T> using DevArr = Arr<T, DeviceMem>;
template <typename T> using PinArr = Arr<T, PinnedMem>;

struct EventOps {
    typedef hipEvent_t handle;
    static hipError_t make(handle* h, unsigned flags) { return hipEventCreateWithFlags(h, flags); }
    static hipError_t destroy(handle h) { return hipEventDestroy(h); }
};
struct StreamOps {
    typedef hipStream_t handle;
    static hipError_t make(handle* h, unsigned flags) { return hipStreamCreateWithFlags(h, flags); }
    static hipError_t destroy(handle h) { return hipStreamDestroy(h); }
};

// One event or one stream.  Creation calls that take more than flags stay where they are and adopt() their handle.
template <class Ops>
class Handle {
    typedef typename Ops::handle H;
    H h_ = nullptr;
    bool owned_ = true;

public:
    Handle() = default;
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    Handle(Handle&& o) noexcept : h_(o.h_), owned_(o.owned_) { o.forget(); }
    Handle& operator=(Handle&& o) noexcept
    {
        if (this != &o) { reset(); h_ = o.h_; owned_ = o.owned_; o.forget(); }
        return *this;
    }
    ~Handle() { reset(); }

    hipError_t create(unsigned flags)                    // an EMPTY owner; a failure leaves it empty
    {
        if (h_) return hipErrorInvalidValue;
        H h = nullptr;
        const hipError_t e = Ops::make(&h, flags);
        if (e == hipSuccess) { h_ = h; owned_ = true; }
        return e;
    }
    hipError_t reset_checked()
    {
        const hipError_t e = h_ && owned_ ? Ops::destroy(h_) : hipSuccess;
        forget();
        return e;
    }
    void reset() { (void)reset_checked(); }
    void adopt(H h) { reset(); h_ = h; owned_ = true; }       // created elsewhere, destroyed here
    void borrow(H h) { reset(); h_ = h; owned_ = false; }     // the caller's: never destroyed

    bool owned() const { return owned_; }
    operator H() const { return h_; }

private:
    void forget() { h_ = nullptr; owned_ = true; }
};

typedef Handle<EventOps> Event;
typedef Handle<StreamOps> Stream;

}  // namespace gd_own
