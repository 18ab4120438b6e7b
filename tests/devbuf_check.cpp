// The failure path of bcm3_amd/csrc/dev_buf.h, on a machine without a HIP device: there every
// allocation fails, which no test on a GPU can arrange. What is checked is the rule the owners of
// device memory rest on: after any call a buffer is (valid pointer, true capacity) or (null, 0),
// so a failed growth can be tried again and the owner destroyed without a second free.
// (tests/test_devbuf.py builds and runs this.)
#include <cstdio>
#include <utility>

#include "../bcm3_amd/csrc/dev_buf.h"

using namespace bcm3hip;

static int failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "devbuf_check:%d: %s\n", __LINE__, #x);     \
            failures++;                                                 \
        }                                                               \
    } while (0)

template <class B>
static void failed_growth()
{
    B b;
    CHECK(b.data() == nullptr && b.capacity() == 0);
    CHECK(b.grow(300, 256) == BCM3HIP_ERR_ALLOC);
    CHECK(b.data() == nullptr && b.capacity() == 0);
    CHECK(b.grow(1) == BCM3HIP_ERR_ALLOC);  // again, and then out of scope: nothing to free twice
    CHECK(b.data() == nullptr && b.capacity() == 0);
    CHECK(b.grow(0) == 0);  // nothing asked for: no allocation, no failure
    b.reset();
    CHECK(b.data() == nullptr && b.capacity() == 0);
}

static int upload3(ModelArrays& arena, const double** dev)
{
    const double host[3] = {1.0, 2.0, 3.0};
    return arena.upload(host, 3, dev);
}

int main()
{
    int count = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && count > 0) {
        fprintf(stderr, "devbuf_check: a HIP device is present; this program checks the no-device case\n");
        return 2;
    }
    failed_growth<DevBuf<double>>();
    failed_growth<PinnedBuf<int32_t>>();
    {
        DevBuf<double> a;
        CHECK(a.grow(8) != 0);
        DevBuf<double> b(std::move(a));
        CHECK(a.data() == nullptr && a.capacity() == 0);
        CHECK(b.data() == nullptr && b.capacity() == 0);
        DevBuf<double> c;
        c = std::move(b);
        CHECK(b.data() == nullptr && b.capacity() == 0);
        CHECK(static_cast<double*>(c) == nullptr);
    }
    {
        ModelArrays arena;
        const double* dev = (const double*)&arena;  // any non-null value
        CHECK(upload3(arena, &dev) == BCM3HIP_ERR_HIP);
        CHECK(dev == nullptr && arena.failed());
        CHECK(arena.upload((const double*)nullptr, 3, &dev) == BCM3HIP_ERR_ARG);
        CHECK(arena.upload((const double*)nullptr, 0, &dev) == 0 && dev == nullptr);
        CHECK(arena.upload_min8((const double*)nullptr, 0) == nullptr);
    }  // the arena goes out of scope with nothing in it
    if (failures == 0) printf("devbuf_check ok\n");
    return failures ? 1 : 0;
}
