// fid_devmem.h -- how the host side of a feature holds device (and pinned host) memory: a layout that cuts one block into typed
// buffers, and an owner of one block that only grows.  A feature allocates ONE block for what it needs and publishes it on the
// context after the allocation has succeeded, so that "some of its buffers exist" is not a state the context can be in.
//
// No HIP call outside fid_mem_alloc / fid_mem_free: with FID_DEVMEM_HOST_TEST defined those two are malloc / free that can be told
// to fail the k-th allocation, and the header compiles with a plain C++ compiler (tests/devmem_main.cpp).
#pragma once

#include <stddef.h>

#include <vector>

#ifdef FID_DEVMEM_HOST_TEST
#include <stdlib.h>
typedef int fid_mem_err;  // 0: done
namespace fid_devmem_test {
inline int fail_in = 0;  // k > 0: the k-th allocation from now fails (and the count stops); 0: none does
inline int allocs = 0;   // allocations that succeeded
}  // namespace fid_devmem_test
inline fid_mem_err fid_mem_alloc(void **p, size_t bytes, bool)
{
    if (fid_devmem_test::fail_in > 0 && --fid_devmem_test::fail_in == 0) return 2;
    *p = malloc(bytes ? bytes : 1);
    fid_devmem_test::allocs += *p != nullptr;
    return *p ? 0 : 2;
}
inline void fid_mem_free(void *p, bool) { free(p); }
#else
#include <hip/hip_runtime.h>
typedef hipError_t fid_mem_err;
inline fid_mem_err fid_mem_alloc(void **p, size_t bytes, bool pinned)
{
    return pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
}
inline void fid_mem_free(void *p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
#endif

// One block cut into buffers, in the order of the add()s.  Every buffer starts on a multiple of 256 bytes (hipMalloc's own alignment,
// which the kernels' 16-byte accesses rely on); a buffer of 0 bytes takes no room.  The same add()s give the same offsets, whatever
// block they are bound to: a device block and its pinned twin, the slabs of two contexts of one size.
struct MemLayout {
    struct Slot {
        void **p;
        size_t off;
    };
    std::vector<Slot> slots;
    size_t end = 0;
    void add_bytes(void **slot, size_t bytes)
    {
        slots.push_back({slot, end});
        end += (bytes + 255) & ~(size_t)255;
    }
    template <class T>
    void add(T **slot, size_t count)
    {
        add_bytes((void **)slot, count * sizeof(T));
    }
    size_t mark() const { return end; }   // where the next buffer will start: two marks bracket the buffers added between them
    size_t bytes() const { return end; }  // the block the layout needs
    void bind(void *base) const
    {
        for (const Slot &s : slots) *s.p = (char *)base + s.off;
    }
};

// One block of device (or pinned host) memory that grows and is then reused: reserve() leaves a block of at least `bytes`, allocating
// only when it has less -- what it held is gone then.  A failed allocation leaves it empty.
template <bool PINNED>
struct MemBlock {
    char *p = nullptr;
    size_t cap = 0;
    MemBlock() = default;
    MemBlock(const MemBlock &) = delete;
    MemBlock &operator=(const MemBlock &) = delete;
    ~MemBlock() { release(); }
    fid_mem_err reserve(size_t bytes)
    {
        if (bytes <= cap) return (fid_mem_err)0;
        release();
        const fid_mem_err e = fid_mem_alloc((void **)&p, bytes, PINNED);
        if (e != (fid_mem_err)0) {
            p = nullptr;
            return e;
        }
        cap = bytes;
        return (fid_mem_err)0;
    }
    void release()
    {
        if (p) fid_mem_free(p, PINNED);
        p = nullptr;
        cap = 0;
    }
};
typedef MemBlock<false> DevBlock;
typedef MemBlock<true> PinnedBlock;

// The same as an array of T.  reserve(count, grown): room for `count` elements; where that takes a new block, one of `grown` elements
// (staging buffers grow in steps, so that a list that gets longer by one does not allocate every time).
template <class T, bool PINNED = false>
struct MemArray {
    MemBlock<PINNED> mem;
    T *data() const { return (T *)mem.p; }
    size_t cap() const { return mem.cap / sizeof(T); }
    fid_mem_err reserve(size_t count) { return mem.reserve(count * sizeof(T)); }
    fid_mem_err reserve(size_t count, size_t grown) { return count > cap() ? mem.reserve(grown * sizeof(T)) : (fid_mem_err)0; }
    void release() { mem.release(); }
};
template <class T>
using DevArray = MemArray<T, false>;
template <class T>
using PinnedArray = MemArray<T, true>;
