// The layout and the owner of fiducials_amd/csrc/fid_devmem.h on the CPU: the allocator seam replaced by malloc / free that can be told
// to fail.  Built with -fsanitize=address,undefined and run by tests/test_devmem.py; exit status 0 and "devmem ok" mean every check held
// (a leak makes the sanitizer end the program with its own status).
#define FID_DEVMEM_HOST_TEST
#include "../fiducials_amd/csrc/fid_devmem.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

static int g_failed = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            g_failed++;                                            \
        }                                                          \
    } while (0)

struct Slots {
    double *a;
    char *b;
    int *none;  // 0 elements
    int16_t *c;
    float *d;
};
static const size_t kBytes[5] = {sizeof(double) * 3, 257, 0, sizeof(int16_t) * 128, sizeof(float) * 1000};

static MemLayout lay(Slots &s, size_t *m0, size_t *m1)
{
    MemLayout l;
    l.add(&s.a, 3);
    *m0 = l.mark();
    l.add(&s.b, 257), l.add(&s.none, 0), l.add(&s.c, 128);
    *m1 = l.mark();
    l.add(&s.d, 1000);
    return l;
}

static void test_layout()
{
    Slots s = {}, t = {};
    size_t m0, m1, n0, n1;
    const MemLayout l = lay(s, &m0, &m1), k = lay(t, &n0, &n1);
    CHECK(l.slots.size() == 5);
    size_t end = 0;
    for (size_t i = 0; i < l.slots.size(); i++) {
        CHECK(l.slots[i].off % 256 == 0);
        CHECK(l.slots[i].off == end);  // in add order, each where the one before ends: none overlaps
        end += (kBytes[i] + 255) / 256 * 256;
        CHECK(l.slots[i].off == k.slots[i].off);  // the same adds, the same offsets
    }
    CHECK(l.bytes() == end && l.mark() == end && k.bytes() == end);
    CHECK(l.slots[2].off == l.slots[3].off);  // 0 bytes advance nothing
    // the marks bracket exactly b, none, c
    CHECK(m0 == l.slots[1].off && m1 == l.slots[4].off && m0 == n0 && m1 == n1);
    CHECK(m1 - m0 == 512 + 0 + 256);
    std::vector<char> block(l.bytes(), 0), other(l.bytes(), 0);
    l.bind(block.data());
    k.bind(other.data());
    char *got[5] = {(char *)s.a, s.b, (char *)s.none, (char *)s.c, (char *)s.d};
    char *got2[5] = {(char *)t.a, t.b, (char *)t.none, (char *)t.c, (char *)t.d};
    for (size_t i = 0; i < 5; i++) {
        CHECK(got[i] == block.data() + l.slots[i].off);
        CHECK(got2[i] == other.data() + l.slots[i].off);
    }
    // every buffer can be written to its end without touching the next one
    memset(s.b, 1, 257);
    memset(s.c, 2, sizeof(int16_t) * 128);
    memset(s.d, 3, sizeof(float) * 1000);
    CHECK(s.b[256] == 1 && ((char *)s.c)[0] == 2 && ((char *)s.c)[255] == 2 && ((char *)s.d)[0] == 3);
}

static void test_owner()
{
    using fid_devmem_test::allocs;
    using fid_devmem_test::fail_in;
    DevBlock b;
    const int a0 = allocs;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(0) == 0 && b.p == nullptr && allocs == a0);
    CHECK(b.reserve(1000) == 0 && b.p && b.cap == 1000 && allocs == a0 + 1);
    memset(b.p, 7, 1000);
    char *p0 = b.p;
    CHECK(b.reserve(10) == 0 && b.p == p0 && b.cap == 1000 && allocs == a0 + 1);    // smaller: reused
    CHECK(b.reserve(1000) == 0 && b.p == p0 && allocs == a0 + 1);
    CHECK(b.reserve(5000) == 0 && b.p && b.cap == 5000 && allocs == a0 + 2);        // larger: a new block
    memset(b.p, 7, 5000);
    fail_in = 1;
    CHECK(b.reserve(6000) != 0 && b.p == nullptr && b.cap == 0 && allocs == a0 + 2);  // failed: empty
    CHECK(fail_in == 0);
    CHECK(b.reserve(100) == 0 && b.p && b.cap == 100 && allocs == a0 + 3);          // ... and usable again
    b.release();
    CHECK(b.p == nullptr && b.cap == 0);
    b.release();
    CHECK(b.p == nullptr && b.cap == 0);
    // the typed forms: counts, growth in steps, pinned
    DevArray<double> arr;
    CHECK(arr.reserve(3, 256) == 0 && arr.cap() == 256 && arr.data());
    double *d0 = arr.data();
    CHECK(arr.reserve(256, 512) == 0 && arr.data() == d0 && arr.cap() == 256);  // fits: no step
    CHECK(arr.reserve(257, 512) == 0 && arr.cap() == 512);
    arr.data()[511] = 1.;
    PinnedArray<int> pin;
    CHECK(pin.reserve(10) == 0 && pin.cap() == 10);
    pin.data()[9] = 1;
    // (arr, pin and what b held are released by their destructors: the sanitizer reports what is not)
}

// "Publish after success" as the features do it: a record is made, allocates its blocks, and is published only when all of them
// exist.  Whichever allocation fails, nothing is published, nothing leaks, and the next call starts from nothing.
struct Feature {
    DevBlock mem;
    PinnedBlock hmem;
    int *d_n = nullptr, *h_n = nullptr;
    double *d_tab = nullptr;
};
static Feature *g_feature = nullptr;

static fid_mem_err feature_ensure()
{
    if (g_feature) return 0;
    Feature *f = new Feature;
    MemLayout dl, hl;
    dl.add(&f->d_n, 17), dl.add(&f->d_tab, 300);
    hl.add(&f->h_n, 17);
    fid_mem_err e = f->mem.reserve(dl.bytes());
    if (e == 0) e = f->hmem.reserve(hl.bytes());
    if (e != 0) {
        delete f;
        return e;
    }
    dl.bind(f->mem.p);
    hl.bind(f->hmem.p);
    g_feature = f;
    return 0;
}

static void test_publish_after_success()
{
    for (int k = 1; k <= 2; k++) {  // the feature makes two allocations: each of them fails once
        fid_devmem_test::fail_in = k;
        CHECK(feature_ensure() != 0);
        CHECK(g_feature == nullptr);
        CHECK(fid_devmem_test::fail_in == 0);
    }
    fid_devmem_test::fail_in = 3;  // (beyond what the feature allocates)
    CHECK(feature_ensure() == 0 && g_feature);
    fid_devmem_test::fail_in = 0;
    if (g_feature) {
        CHECK(g_feature->d_n && g_feature->h_n && g_feature->d_tab);
        g_feature->d_tab[299] = 1.;
        g_feature->d_n[16] = g_feature->h_n[16] = 1;
        Feature *f = g_feature;
        CHECK(feature_ensure() == 0 && g_feature == f);
    }
    delete g_feature;
    g_feature = nullptr;
}

int main()
{
    test_layout();
    test_owner();
    test_publish_after_success();
    if (g_failed) {
        printf("devmem: %d checks failed\n", g_failed);
        return 1;
    }
    printf("devmem ok\n");
    return 0;
}
