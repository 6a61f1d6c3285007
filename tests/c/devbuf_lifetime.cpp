// The rules of csrc/oa_devbuf.hpp's handle, on the host: the header against a counting allocator (tests/test_devbuf_lifetime.py
// builds this with -fsanitize=address,undefined).  Every block is a malloc of its own that stays allocated until main returns, so
// no address comes back and the per-block release counts stay exact.
#include "oa_devbuf.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

namespace {
struct Block { size_t bytes; int releases; int settled; };
std::map<void *, Block> g_blocks;      // every block ever handed out
int g_allocs = 0, g_releases = 0, g_settled = 0, g_failures = 0;
bool g_fail_next = false;

int live_blocks()
{
    int n = 0;
    for (const auto &kv : g_blocks) n += kv.second.releases == 0 ? 1 : 0;
    return n;
}

void check(bool ok, const char *what)
{
    if (!ok) { ++g_failures; std::printf("FAILED: %s\n", what); }
}
}  // namespace

int oa::dev_block_alloc(void **out, size_t bytes)
{
    if (g_fail_next) { g_fail_next = false; return 2; }
    void *p = std::malloc(bytes ? bytes : 1);
    if (!p) return 2;
    g_blocks[p] = Block{ bytes, 0, 0 };
    ++g_allocs;
    *out = p;
    return 0;
}

void oa::dev_block_release(void *p, bool settled)
{
    auto it = g_blocks.find(p);
    check(it != g_blocks.end(), "a released pointer is one the allocator handed out");
    if (it == g_blocks.end()) return;
    check(it->second.releases == 0, "a block is released once");
    ++it->second.releases;
    it->second.settled += settled ? 1 : 0;
    ++g_releases;
    g_settled += settled ? 1 : 0;
}

namespace {
using oa::DevBuf;

// a lifetime group as oa_ctx holds them: handles, flags and counts with default initialisers
struct Group {
    int n = 0;
    bool ok = false;
    DevBuf<float> a;
    DevBuf<int> b;
    DevBuf<double> never;              // stays empty
    long long entries = 0;
    DevBuf<char> c;
    double frame[3] = { 0, 0, 0 };
    std::vector<int> host;
};

void fill(Group &g)
{
    check(g.a.alloc(100) == 0 && g.b.alloc(7) == 0 && g.c.alloc_bytes(33) == 0, "allocations succeed");
    g.n = 100; g.ok = true; g.entries = 1ll << 40; g.frame[1] = 2.5; g.host.assign(5, 9);
}

void test_group_reset()
{
    Group g;
    fill(g);
    const void *pa = g.a.p, *pb = g.b.p, *pc = g.c.p;
    check(live_blocks() == 3 && g_blocks[g.a.p].bytes == 100 * sizeof(float) && g_blocks[g.c.p].bytes == 33, "three live blocks of the sizes asked for");
    const int r0 = g_releases;
    g = {};
    check(g_releases - r0 == 3 && live_blocks() == 0, "= {} releases each live block exactly once");
    check(g_blocks[(void *)pa].releases == 1 && g_blocks[(void *)pb].releases == 1 && g_blocks[(void *)pc].releases == 1, "... every one of them");
    check(!g.a && !g.b && !g.c && !g.never, "= {} leaves every handle empty");
    check(g.n == 0 && !g.ok && g.entries == 0 && g.frame[1] == 0.0 && g.host.empty(), "= {} returns every flag and count to its default");
    g = {};
    check(g_releases - r0 == 3, "= {} on an empty group releases nothing");
    fill(g);
    const int r1 = g_releases;
    {
        Group scoped;
        fill(scoped);
    }
    check(g_releases - r1 == 3, "a group that goes out of scope releases its blocks");
    g = {};
}

void test_move()
{
    DevBuf<int> x;
    check(x.alloc(10) == 0, "alloc");
    int *const p = x.p;
    const int r0 = g_releases;
    DevBuf<int> y(std::move(x));
    check(x.p == nullptr && y.p == p && g_releases == r0, "move construction hands the block over and leaves the source empty");
    DevBuf<int> z;
    check(z.alloc(3) == 0, "alloc");
    int *const old = z.p;
    z = std::move(y);
    check(y.p == nullptr && z.p == p, "move assignment leaves the source empty");
    check(g_releases - r0 == 1 && g_blocks[(void *)old].releases == 1, "... and releases what the destination held");
    DevBuf<int> &same = z;
    z = std::move(same);
    check(z.p == p && g_releases - r0 == 1, "self-assignment keeps the block");
    z.reset();
    check(g_blocks[(void *)p].releases == 1 && live_blocks() == 0, "one release of the moved block in all");
}

void test_alloc_on_live()
{
    DevBuf<double> x;
    check(x.alloc(4) == 0, "alloc");
    double *const first = x.p;
    const int r0 = g_releases;
    check(x.alloc(8) == 0, "second alloc");
    check(g_releases - r0 == 1 && g_blocks[(void *)first].releases == 1 && live_blocks() == 1, "alloc on a live handle releases first");
    check(g_blocks[(void *)x.p].bytes == 8 * sizeof(double), "... and holds the new block");
    check(x.alloc(0) == 0 && g_blocks[(void *)x.p].bytes == sizeof(double), "alloc(0) asks for one element");
    g_fail_next = true;
    check(x.alloc(16) != 0 && x.p == nullptr && live_blocks() == 0, "a failed alloc returns the code and leaves the handle empty");
}

void test_destruction_after_reset()
{
    const int r0 = g_releases;
    {
        DevBuf<float> x;
        check(x.alloc(5) == 0, "alloc");
        x.reset();
        check(g_releases - r0 == 1 && !x, "reset releases and empties");
        x.reset();
        check(g_releases - r0 == 1, "a second reset releases nothing");
    }
    check(g_releases - r0 == 1, "destruction after reset() releases nothing");
    { DevBuf<float> never; }
    check(g_releases - r0 == 1, "an empty handle releases nothing");
}

void test_pointer_view()
{
    DevBuf<float> x;
    check(!x, "an empty handle tests false");
    check(x.alloc(8) == 0, "alloc");
    float *raw = x;
    const float *craw = x;
    check(raw == x.p && craw == x.p && x + 3 == x.p + 3 && (const char *)x == (const char *)x.p && x, "the handle reads as the pointer it holds");
}

void test_teardown_scope()
{
    Group g, h;
    fill(g); fill(h);
    const int s0 = g_settled, r0 = g_releases;
    g = {};
    check(g_releases - r0 == 3 && g_settled == s0, "outside a teardown no release is settled");
    check(!oa::DevTeardown::active(), "no teardown is active by default");
    {
        oa::DevTeardown down;
        check(oa::DevTeardown::active(), "the scope marks this thread");
        {
            oa::DevTeardown inner;
        }
        check(oa::DevTeardown::active(), "a nested scope's end does not end the outer one");
        h = {};
        DevBuf<int> t;
        check(t.alloc(2) == 0, "alloc");
    }
    check(g_releases - r0 == 7 && g_settled - s0 == 4, "every release inside a teardown is settled");
    check(!oa::DevTeardown::active(), "the scope's end ends it");
    DevBuf<int> after;
    check(after.alloc(2) == 0, "alloc");
    after.reset();
    check(g_settled - s0 == 4, "... and the releases behind it are not settled");
}
}  // namespace

int main()
{
    test_group_reset();
    test_move();
    test_alloc_on_live();
    test_destruction_after_reset();
    test_pointer_view();
    test_teardown_scope();
    check(live_blocks() == 0 && g_allocs == g_releases, "every block handed out came back, once");
    for (const auto &kv : g_blocks) std::free(kv.first);
    std::printf("%d allocations, %d releases (%d settled), %d checks failed\n", g_allocs, g_releases, g_settled, g_failures);
    return g_failures ? 1 : 0;
}
