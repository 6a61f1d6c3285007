// sort_check.hip -- the index builds' primitives run on caller-supplied inputs: the stable argsorts (oa_sort.hpp: k_sort_small,
// the LSD passes), the orders by several keys (lex_order_next), the prefix sums (scan_counts_ll; k_scan_counts of oa_kernels.hpp, launched as oa_make_pairs does) and
// k_gather_int.  It holds no reference and makes no inputs: it reads them from files, runs the library's code on the device and
// writes what the device returned; tests/test_gpu_index_primitives.py compares that with numpy.
// build: __graft_entry__.build_tools()     run: tools/sort_check.exe MANIFEST
// MANIFEST: one case per line (paths without blanks; '#' starts a comment line)
//   sort auto|lsd BITS N KEYS OUT      uint32 keys[N] -> int32 order[N]        auto: oa::sort_order, lsd: oa::sort_order_lsd whatever N
//   lex NKEYS N BITS.. KEYS.. OUT      NKEYS widths, then NKEYS files of uint32 keys[N], the LEAST significant key first -> int32 order[N]:
//                                      oa::sort_order on the first key, oa::lex_order_next once per further key
//   scan ll|block N COUNTS OUT        int32 counts[N] -> int64 offsets[N + 1] ll: oa::scan_counts_ll, block: oa::k_scan_counts <<<1, 1024>>>
//   gather NSRC N SRC IDX OUT          int32 src[NSRC], idx[N] -> int32 out[N] oa::k_gather_int with sort_ints' launch shape
// Every device output, and the temporary buffer of exactly sort_order_tmp_bytes(N) / lex_order_tmp_bytes(N) / scan_tmp_bytes(N)
// bytes, lies between two guard zones filled with a byte pattern that must survive the run; the inputs are read back and must be
// unchanged (lex_order_next overwrites its keys: it gets a guarded copy, the input stays).  One line
// per case with the verdicts; the first HIP error or violated guard ends the process with a non-zero status.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "oa_kernels.hpp"
#include "oa_sort.hpp"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error: %s (%s, line %d)\n", hipGetErrorString(e_), #x, __LINE__); fflush(stdout); exit(3); } } while (0)

static const size_t GUARD = 65536;                                   // bytes on either side of a guarded buffer
static const unsigned char PATTERN = 0xA5;

static void die(int line_no, const char *what)
{
    printf("case %d: %s\n", line_no, what);
    fflush(stdout);
    exit(2);
}

// `bytes` of device memory between two guard zones, all of it (the payload included) filled with PATTERN
struct Guarded {
    unsigned char *base = nullptr;
    size_t bytes = 0;
    explicit Guarded(size_t n) : bytes(n)
    {
        CHK(hipMalloc((void **)&base, n + 2 * GUARD));
        CHK(hipMemset(base, PATTERN, n + 2 * GUARD));
    }
    void *p() const { return base + GUARD; }
    // the guard zones after the run; `payload` (optional) receives the bytes between them
    bool intact(void *payload) const
    {
        std::vector<unsigned char> h(bytes + 2 * GUARD);
        CHK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        if (payload && bytes) memcpy(payload, h.data() + GUARD, bytes);
        for (size_t i = 0; i < GUARD; ++i)
            if (h[i] != PATTERN || h[GUARD + bytes + i] != PATTERN) return false;
        return true;
    }
    ~Guarded() { (void)hipFree(base); }
    Guarded(const Guarded &) = delete;
    Guarded &operator=(const Guarded &) = delete;
};

// an input: the file's n elements on the device, and the host copy they are compared with afterwards
template <class T>
struct Input {
    std::vector<T> host;
    T *dev = nullptr;
    Input(int line_no, const char *path, size_t n) : host(n)
    {
        FILE *f = fopen(path, "rb");
        if (!f) die(line_no, "cannot open an input file");
        const size_t got = n ? fread(host.data(), sizeof(T), n, f) : 0;
        const bool more = fgetc(f) != EOF;
        fclose(f);
        if (got != n || more) die(line_no, "an input file does not hold exactly N elements");
        CHK(hipMalloc((void **)&dev, sizeof(T) * (n ? n : 1)));
        if (n) CHK(hipMemcpy(dev, host.data(), sizeof(T) * n, hipMemcpyHostToDevice));
    }
    bool untouched() const
    {
        std::vector<T> now(host.size());
        if (!now.empty()) CHK(hipMemcpy(now.data(), dev, sizeof(T) * now.size(), hipMemcpyDeviceToHost));
        return now.empty() || memcmp(now.data(), host.data(), sizeof(T) * now.size()) == 0;
    }
    ~Input() { (void)hipFree(dev); }
    Input(const Input &) = delete;
    Input &operator=(const Input &) = delete;
};

static void write_file(int line_no, const char *path, const void *data, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f) die(line_no, "cannot open the output file");
    const size_t put = bytes ? fwrite(data, 1, bytes, f) : 0;
    if (fclose(f) != 0 || put != bytes) die(line_no, "cannot write the output file");
}

// the verdicts of a case: prints them, ends the process on a violated one
static void verdict(int line_no, const char *what, size_t n, bool guards, bool inputs)
{
    printf("case %d %s n=%zu: guards %s inputs %s\n", line_no, what, n, guards ? "ok" : "VIOLATED", inputs ? "untouched" : "CHANGED");
    fflush(stdout);
    if (!guards || !inputs) exit(1);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s MANIFEST\n", argv[0]); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[8192];
    int line_no = 0, cases = 0;
    const long long n_max = 1ll << 26;                               // (the kernels take n as int; nothing here comes near)
    while (fgets(line, sizeof line, mf)) {
        ++line_no;
        char mode[16], sub[16], f0[2048], f1[2048], f2[2048];
        if (line[0] == '#' || line[0] == '\n') continue;
        if (sscanf(line, "%15s", mode) != 1) continue;
        if (strcmp(mode, "sort") == 0) {
            int bits; long long n;
            if (sscanf(line, "%*s %15s %d %lld %2047s %2047s", sub, &bits, &n, f0, f1) != 5) die(line_no, "malformed sort line");
            const bool lsd = strcmp(sub, "lsd") == 0;
            if ((!lsd && strcmp(sub, "auto") != 0) || bits < 1 || bits > 32 || n < 0 || n > n_max) die(line_no, "bad sort arguments");
            Input<uint32_t> keys(line_no, f0, (size_t)n);
            Guarded tmp(oa::sort_order_tmp_bytes((size_t)n)), order(sizeof(int) * (size_t)n);
            if (lsd) CHK(oa::sort_order_lsd(tmp.p(), keys.dev, (int *)order.p(), (size_t)n, bits, 0));
            else CHK(oa::sort_order(tmp.p(), keys.dev, (int *)order.p(), (size_t)n, bits, 0));
            CHK(hipDeviceSynchronize());
            std::vector<int> h((size_t)n);
            const bool g_out = order.intact(h.data()), g_tmp = tmp.intact(nullptr);
            write_file(line_no, f1, h.data(), sizeof(int) * h.size());
            verdict(line_no, lsd ? "sort lsd" : "sort auto", (size_t)n, g_out && g_tmp, keys.untouched());
        } else if (strcmp(mode, "lex") == 0) {
            int nk = 0; long long n = 0;
            std::istringstream words(line);
            std::string word;
            words >> word >> nk >> n;
            if (!words || nk < 1 || nk > 8 || n < 1 || n > n_max) die(line_no, "bad lex arguments");
            std::vector<int> bits((size_t)nk);
            std::vector<std::string> paths((size_t)nk + 1);
            for (int &b : bits) { words >> b; if (!words || b < 1 || b > 32) die(line_no, "bad lex key width"); }
            for (std::string &p : paths) if (!(words >> p)) die(line_no, "malformed lex line");
            // key 0 is only read; a later key is the stage's scratch, so the function gets a guarded copy of it
            std::vector<std::unique_ptr<Input<uint32_t>>> keys;
            std::vector<std::unique_ptr<Guarded>> scratch;
            for (int k = 0; k < nk; ++k) {
                keys.emplace_back(new Input<uint32_t>(line_no, paths[(size_t)k].c_str(), (size_t)n));
                if (k == 0) continue;
                scratch.emplace_back(new Guarded(sizeof(uint32_t) * (size_t)n));
                CHK(hipMemcpy(scratch.back()->p(), keys.back()->dev, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice));
            }
            Guarded tmp(oa::lex_order_tmp_bytes((size_t)n)), ord_a(sizeof(int) * (size_t)n), ord_b(sizeof(int) * (size_t)n);
            Guarded *cur = &ord_a, *other = &ord_b;
            CHK(oa::sort_order(tmp.p(), keys[0]->dev, (int *)cur->p(), (size_t)n, bits[0], 0));
            for (int k = 1; k < nk; ++k) {
                CHK(oa::lex_order_next(tmp.p(), (uint32_t *)scratch[(size_t)k - 1]->p(), bits[(size_t)k], (const int *)cur->p(), (int *)other->p(), (size_t)n, 0));
                std::swap(cur, other);
            }
            CHK(hipDeviceSynchronize());
            std::vector<int> h((size_t)n);
            bool guards = cur->intact(h.data()) && other->intact(nullptr) && tmp.intact(nullptr), inputs = true;
            for (const auto &s : scratch) guards = guards && s->intact(nullptr);
            for (const auto &k : keys) inputs = inputs && k->untouched();
            write_file(line_no, paths[(size_t)nk].c_str(), h.data(), sizeof(int) * h.size());
            verdict(line_no, "lex", (size_t)n, guards, inputs);
        } else if (strcmp(mode, "scan") == 0) {
            long long n;
            if (sscanf(line, "%*s %15s %lld %2047s %2047s", sub, &n, f0, f1) != 4) die(line_no, "malformed scan line");
            const bool block = strcmp(sub, "block") == 0;
            if ((!block && strcmp(sub, "ll") != 0) || n < 0 || n > n_max) die(line_no, "bad scan arguments");
            Input<int> counts(line_no, f0, (size_t)n);
            Guarded tmp(oa::scan_tmp_bytes((size_t)n)), offsets(sizeof(long long) * (size_t)(n + 1));
            if (block) {
                hipLaunchKernelGGL(oa::k_scan_counts, dim3(1), dim3(1024), 0, 0, (const int *)counts.dev, (int)n, (long long *)offsets.p());
                CHK(hipGetLastError());
            } else CHK(oa::scan_counts_ll(tmp.p(), counts.dev, (size_t)n, (long long *)offsets.p(), 0));
            CHK(hipDeviceSynchronize());
            std::vector<long long> h((size_t)n + 1);
            const bool g_out = offsets.intact(h.data()), g_tmp = tmp.intact(nullptr);
            write_file(line_no, f1, h.data(), sizeof(long long) * h.size());
            verdict(line_no, block ? "scan block" : "scan ll", (size_t)n, g_out && g_tmp, counts.untouched());
        } else if (strcmp(mode, "gather") == 0) {
            long long n_src, n;
            if (sscanf(line, "%*s %lld %lld %2047s %2047s %2047s", &n_src, &n, f0, f1, f2) != 5) die(line_no, "malformed gather line");
            if (n_src < 1 || n_src > n_max || n < 1 || n > n_max) die(line_no, "bad gather arguments");
            Input<int> src(line_no, f0, (size_t)n_src), idx(line_no, f1, (size_t)n);
            for (int i : idx.host) if (i < 0 || i >= n_src) die(line_no, "an index outside src");   // (the kernel trusts its indices)
            Guarded out(sizeof(int) * (size_t)n);
            hipLaunchKernelGGL(oa::k_gather_int, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const int *)src.dev, (const int *)idx.dev, (int)n, (int *)out.p());
            CHK(hipGetLastError());
            CHK(hipDeviceSynchronize());
            std::vector<int> h((size_t)n);
            const bool g_out = out.intact(h.data());
            write_file(line_no, f2, h.data(), sizeof(int) * h.size());
            verdict(line_no, "gather", (size_t)n, g_out, src.untouched() && idx.untouched());
        } else die(line_no, "unknown mode");
        ++cases;
    }
    fclose(mf);
    printf("%d cases done\n", cases);
    return 0;
}
