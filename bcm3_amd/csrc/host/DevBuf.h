// DevBuf.h -- a device array of the host samplers, owned through libbcm3hip's C ABI
// (bcm3hip_malloc / bcm3hip_free): this library is built without the HIP headers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "../../../include/bcm3hip.h"

namespace bcm3 {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;  // elements asked for (at least one is allocated)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    bool alloc(size_t count)
    {
        n = count;
        return bcm3hip_malloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)) == 0;
    }
    ~DevBuf() { bcm3hip_free(p); }
};

template <class T>
bool Upload(DevBuf<T>& b, const std::vector<T>& h, void* s)
{
    return bcm3hip_memcpy_async(b.p, h.data(), h.size() * sizeof(T), BCM3HIP_H2D, s) == 0;
}
template <class T>
bool Download(std::vector<T>& h, const DevBuf<T>& b, void* s)
{
    h.resize(b.n);
    return bcm3hip_memcpy_async(h.data(), b.p, b.n * sizeof(T), BCM3HIP_D2H, s) == 0 && bcm3hip_stream_synchronize(s) == 0;
}

}  // namespace bcm3
