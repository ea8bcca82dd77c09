// The four owners of goleft_amd/csrc/gd_own.hpp on the host alone, for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_own_asan.py): this program IS the HIP runtime they see -- the eight functions below over malloc, counting
// what lives per kind, refusing a free of what does not live, failing the k-th creation on request.
#include "gd_own.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {

enum Kind { DEV, PIN, EVENT, STREAM, KINDS };
std::set<void*> live[KINDS];
long made[KINDS], gone[KINDS];
long wrong_frees = 0;            // a pointer that was not live in its kind: freed twice, or never allocated
long fail_in = 0;                // > 0: the fail_in-th creation from now fails
bool fail_next_free = false;
size_t last_bytes = 0;
void* last_gone = nullptr;

hipError_t make(Kind k, void** out, size_t bytes)
{
    if (fail_in > 0 && --fail_in == 0) return hipErrorOutOfMemory;
    void* p = malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    live[k].insert(p);
    ++made[k];
    last_bytes = bytes;
    *out = p;
    return hipSuccess;
}

hipError_t drop(Kind k, void* p)
{
    if (fail_next_free) { fail_next_free = false; return hipErrorInvalidValue; }
    if (!live[k].erase(p)) { ++wrong_frees; return hipErrorInvalidValue; }
    ++gone[k];
    last_gone = p;
    free(p);
    return hipSuccess;
}

long frees() { return gone[DEV] + gone[PIN] + gone[EVENT] + gone[STREAM]; }

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return make(DEV, p, n); }
hipError_t hipFree(void* p) { return drop(DEV, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return make(PIN, p, n); }
hipError_t hipHostFree(void* p) { return drop(PIN, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(EVENT, reinterpret_cast<void**>(e), 8); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(EVENT, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return make(STREAM, reinterpret_cast<void**>(s), 8); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(STREAM, s); }
}

#define CHECK(x)                                                                  \
    do {                                                                          \
        if (!(x)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; }    \
    } while (0)

// what holds for a device array and for a page-locked one alike
template <class A, Kind K>
int arrays()
{
    typedef decltype(A().get()) P;
    {   // construction and destruction; the bytes asked for; a count of 0 is one element
        A a;
        CHECK(!a && a.get() == nullptr && a.cap() == 0);
        CHECK(a.alloc(10) == hipSuccess && a && a.cap() == 10 && last_bytes == 10 * sizeof(*a.get()) && live[K].size() == 1);
        a.get()[9] = a.get()[0];                       // (the block is that large)
        A z;
        CHECK(z.alloc(0) == hipSuccess && z.cap() == 1 && last_bytes == sizeof(*z.get()) && live[K].size() == 2);
    }
    CHECK(live[K].empty());
    {   // a move leaves the source empty and frees nothing
        A a;
        CHECK(a.alloc(7) == hipSuccess);
        const P p = a.get();
        const long f = frees();
        A b(std::move(a));
        CHECK(!a && a.cap() == 0 && b.get() == p && b.cap() == 7 && frees() == f);
        // move-assignment onto a full owner frees exactly the old block
        A c;
        CHECK(c.alloc(3) == hipSuccess);
        const P old = c.get();
        c = std::move(b);
        CHECK(frees() == f + 1 && last_gone == old && c.get() == p && c.cap() == 7 && !b && live[K].size() == 1);
        // ... and onto an empty one nothing
        A d;
        d = std::move(c);
        CHECK(frees() == f + 1 && d.get() == p && !c);
        // reset is idempotent
        d.reset();
        CHECK(frees() == f + 2 && !d && d.cap() == 0);
        d.reset();
        CHECK(d.reset_checked() == hipSuccess && frees() == f + 2);
    }
    CHECK(live[K].empty());
    {   // reset_checked reports what the runtime says, and the owner is empty either way
        A a;
        CHECK(a.alloc(2) == hipSuccess);
        void* p = a.get();
        fail_next_free = true;
        CHECK(a.reset_checked() == hipErrorInvalidValue && !a && a.cap() == 0);
        CHECK(drop(K, p) == hipSuccess);                // (the stand-in kept it: give it back)
    }
    {   // release hands the block out, and the owner then frees nothing
        const long f = frees();
        P p = nullptr;
        {
            A a;
            CHECK(a.alloc(5) == hipSuccess);
            p = a.release();
            CHECK(p && !a && a.cap() == 0);
        }
        CHECK(frees() == f && live[K].count(p) == 1);
        // a borrowed block is never freed: not by the destructor, a reset, a move or a move-assignment
        {
            A b;
            b.borrow(p, 5);
            CHECK(b.get() == p && b.cap() == 5);
            A c(std::move(b));
            CHECK(!b && c.get() == p);
            A d;
            d.borrow(p, 5);
            d = std::move(c);
            d.reset();
            d.borrow(p, 5);
            A e;
            CHECK(e.alloc(1) == hipSuccess);
            e.borrow(p, 5);                            // (the owner's own block goes first)
            CHECK(frees() == f + 1 && live[K].size() == 1);
        }
        CHECK(frees() == f + 1 && live[K].count(p) == 1);
        CHECK(drop(K, p) == hipSuccess);
    }
    {   // a failed allocation leaves the owner empty; alloc on a full owner is refused and changes nothing
        A a;
        fail_in = 1;
        CHECK(a.alloc(4) == hipErrorOutOfMemory && !a && a.cap() == 0 && live[K].empty());
        CHECK(a.alloc(4) == hipSuccess);
        const P p = a.get();
        const long f = frees(), m = made[K];
        CHECK(a.alloc(9) == hipErrorInvalidValue && a.get() == p && a.cap() == 4 && frees() == f && made[K] == m);
        // a creation that fails beside a full owner: that one is still freed once, when it goes
        A b;
        fail_in = 1;
        CHECK(b.alloc(4) == hipErrorOutOfMemory && !b);
    }
    CHECK(live[K].empty());
    return 0;
}

template <class Hd, class Raw, Kind K>
int handles()
{
    {   // construction and destruction; create on a full owner is refused
        Hd h;
        CHECK(!h);
        CHECK(h.create(0) == hipSuccess && h && h.owned() && live[K].size() == 1);
        const Raw raw = h;
        CHECK(h.create(0) == hipErrorInvalidValue && Raw(h) == raw && live[K].size() == 1);
    }
    CHECK(live[K].empty());
    {   // a failed creation leaves it empty; moves, move-assignment and reset as for the arrays
        Hd a;
        fail_in = 1;
        CHECK(a.create(0) != hipSuccess && !a && live[K].empty());
        CHECK(a.create(0) == hipSuccess);
        const Raw raw = a;
        const long f = frees();
        Hd b(std::move(a));
        CHECK(!a && Raw(b) == raw && frees() == f);
        Hd c;
        CHECK(c.create(0) == hipSuccess);
        const Raw old = c;
        c = std::move(b);
        CHECK(frees() == f + 1 && last_gone == old && !b && Raw(c) == raw && live[K].size() == 1);
        c.reset();
        c.reset();
        CHECK(c.reset_checked() == hipSuccess && frees() == f + 2 && live[K].empty());
    }
    {   // a handle created elsewhere: borrowed, it is never destroyed; adopted, once
        Raw theirs = nullptr;
        CHECK(make(K, reinterpret_cast<void**>(&theirs), 8) == hipSuccess);
        const long f = frees();
        {
            Hd b;
            b.borrow(theirs);
            CHECK(Raw(b) == theirs && !b.owned());
            Hd c(std::move(b));
            Hd d;
            CHECK(d.create(0) == hipSuccess);
            d = std::move(c);                          // (d's own handle goes, the borrowed one moves in)
            CHECK(frees() == f + 1 && Raw(d) == theirs && !d.owned());
            d.reset();
            CHECK(d.owned());                          // (empty again: what it creates next is its own)
            d.borrow(theirs);
            CHECK(d.reset_checked() == hipSuccess);
            d.borrow(theirs);
        }
        CHECK(frees() == f + 1 && live[K].count(theirs) == 1);
        {
            Hd a;
            CHECK(a.create(0) == hipSuccess);
            a.adopt(theirs);                           // (its own goes first)
            CHECK(frees() == f + 2 && a.owned() && Raw(a) == theirs);
        }
        CHECK(frees() == f + 3 && live[K].empty());
    }
    return 0;
}

int main()
{
    using namespace gd_own;
    if (arrays<DevArr<int>, DEV>()) return 1;
    if (arrays<DevArr<double>, DEV>()) return 1;
    if (arrays<PinArr<unsigned char>, PIN>()) return 1;
    if (arrays<PinArr<long long>, PIN>()) return 1;
    CHECK(DevArr<unsigned char>().as<int>() == nullptr);
    if (handles<Event, hipEvent_t, EVENT>()) return 1;
    if (handles<Stream, hipStream_t, STREAM>()) return 1;
    for (int k = 0; k < KINDS; ++k) CHECK(live[k].empty() && made[k] == gone[k] && made[k] > 0);
    CHECK(wrong_frees == 0);
    printf("ok\n");
    return 0;
}
