// dev_buf.h -- who owns the device memory of libbcm3hip.so (library-internal; .cpp / .hip only).
//
//   DevBuf<T>      one grow-only buffer; after any call it is (valid pointer, true capacity) or
//                  (null, 0), and its destructor frees it
//   PinnedBuf<T>   the same in pinned host memory
//   ModelArrays    the model arrays uploaded once per context, freed with it
//   HIPCHK_AS      the error macro of the host files
//
// Every free goes to the current device: select the owner's device before it is destroyed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/bcm3hip.h"

// a failed HIP call: one line on stderr under the file's prefix, BCM3HIP_ERR_HIP to the caller
#define HIPCHK_AS(prefix, x)                                                                               \
    do {                                                                                                   \
        hipError_t e_ = (x);                                                                               \
        if (e_ != hipSuccess) {                                                                            \
            fprintf(stderr, prefix ": %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return BCM3HIP_ERR_HIP;                                                                        \
        }                                                                                                  \
    } while (0)

namespace bcm3hip {

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void release(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem = DeviceMem>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // Room for `need` elements, at least `floor` when it has to allocate. The contents are NOT
    // preserved: the old allocation is freed before the new one is made, so the peak is the larger
    // of the two and not their sum. 0, or BCM3HIP_ERR_ALLOC with the buffer left empty.
    int grow(size_t need, size_t floor = 1)
    {
        if (need <= cap_) return 0;
        reset();
        const size_t n = need < floor ? floor : need;
        void* p = nullptr;
        if (Mem::alloc(&p, n * sizeof(T)) != hipSuccess || !p) return BCM3HIP_ERR_ALLOC;
        p_ = (T*)p;
        cap_ = n;
        return 0;
    }
    void reset()
    {
        if (p_) Mem::release(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T* data() const { return p_; }
    size_t capacity() const { return cap_; }  // in elements
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T>
using PinnedBuf = DevBuf<T, PinnedMem>;

class ModelArrays {
public:
    ModelArrays() = default;
    ModelArrays(const ModelArrays&) = delete;
    ModelArrays& operator=(const ModelArrays&) = delete;
    ~ModelArrays()
    {
        for (void* p : allocs_) (void)hipFree(p);
    }

    // host[count] on the device in *dev_out. count == 0: a null device pointer; a null host pointer
    // with count > 0: BCM3HIP_ERR_ARG
    template <class T>
    int upload(const T* host, size_t count, const T** dev_out)
    {
        *dev_out = nullptr;
        if (count == 0) return 0;
        if (!host) return BCM3HIP_ERR_ARG;
        void* p = nullptr;
        HIPCHK_AS("bcm3hip", device_malloc(&p, count * sizeof(T)));
        HIPCHK_AS("bcm3hip", hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
        *dev_out = (const T*)p;
        return 0;
    }
    // the same for arrays that may be empty or absent: at least 8 bytes, so the device pointer is
    // valid either way; null when the allocation fails, which failed() remembers
    template <class T>
    T* upload_min8(const T* host, size_t count)
    {
        const size_t bytes = count * sizeof(T);
        void* p = nullptr;
        if (device_malloc(&p, bytes < 8 ? 8 : bytes) != hipSuccess) return nullptr;
        if (count && host) (void)hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        return (T*)p;
    }
    bool failed() const { return failed_; }

private:
    hipError_t device_malloc(void** p, size_t bytes)
    {
        *p = nullptr;
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess && *p)
            allocs_.push_back(*p);
        else
            failed_ = true;
        return e;
    }
    std::vector<void*> allocs_;
    bool failed_ = false;
};

}  // namespace bcm3hip
