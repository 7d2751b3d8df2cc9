// addr_host_bench.cpp -- the scalar host ABI of include/hyobfs_addr.h on T threads: what
// the same work costs without a GPU, next to scripts/bench_addr.py's device legs.
//
// ITEMS (scripts/bench_addr.py writes it, little-endian): u64 n, u64 buf_len, u64 off[n],
// u32 len[n], the text buffer, then for the format leg 16 n bytes of addresses, n family
// bytes and n u16 ports.  The items are split evenly over T threads, which run
//   parse   hyobfs_addr_parse per text
//   format  hyobfs_addr_format per address
// REPS times each; the time of a leg is the median over the repetitions of the wall time
// from a common start until the last thread is done.  Prints one JSON line.
//
//   g++ -O2 -std=c++17 tools/addr_host_bench.cpp -o tools/addr_host_bench -ldl -lpthread
//   tools/addr_host_bench hysteria_amd/libhyobfs.so ITEMS [T = 16] [REPS = 5]
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../include/hyobfs_addr.h"

typedef int (*parse_fn)(const uint8_t*, size_t, uint32_t*, uint32_t*, uint8_t*, uint8_t*, uint8_t*, uint16_t*);
typedef int (*format_fn)(const uint8_t*, uint32_t, uint16_t, uint8_t*, size_t);

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <class F>
static double leg(int T, int reps, uint64_t n, F body) {
    std::vector<double> ms;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back([&, t] { body(n * t / T, n * (t + 1) / T); });
        for (auto& x : th) x.join();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s LIBHYOBFS ITEMS [T] [REPS]\n", argv[0]);
        return 2;
    }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) {
        fprintf(stderr, "%s\n", dlerror());
        return 2;
    }
    const parse_fn parse = (parse_fn)dlsym(lib, "hyobfs_addr_parse");
    const format_fn format = (format_fn)dlsym(lib, "hyobfs_addr_format");
    FILE* f = fopen(argv[2], "rb");
    if (!parse || !format || !f) return 2;
    const int T = argc > 3 ? atoi(argv[3]) : 16, reps = argc > 4 ? atoi(argv[4]) : 5;
    uint64_t n = 0, buf_len = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> buf, ip, family;
    std::vector<uint16_t> port;
    if (fread(&n, 8, 1, f) != 1 || fread(&buf_len, 8, 1, f) != 1 || !rd(f, off, n) || !rd(f, len, n) || !rd(f, buf, buf_len) ||
        !rd(f, ip, 16 * n) || !rd(f, family, n) || !rd(f, port, n) || T < 1 || reps < 1)
        return 2;
    fclose(f);
    std::atomic<uint64_t> ok{0}, bytes{0};   // summed over the repetitions
    const double parse_ms = leg(T, reps, n, [&](uint64_t a, uint64_t b) {
        uint64_t good = 0;
        for (uint64_t i = a; i < b; ++i) {
            uint32_t no, nl;
            uint8_t v4[4], v6[16], fl;
            uint16_t p;
            good += parse(buf.data() + off[i], len[i], &no, &nl, v4, v6, &fl, &p) == HYOBFS_OK;
        }
        ok += good;
    });
    const double format_ms = leg(T, reps, n, [&](uint64_t a, uint64_t b) {
        uint64_t total = 0;
        uint8_t out[HYOBFS_ADDR_FORMAT_MAX];
        for (uint64_t i = a; i < b; ++i) {
            const int r = format(ip.data() + 16 * i, family[i], port[i], out, sizeof out);
            total += r > 0 ? (uint64_t)r : 0;
        }
        bytes += total;
    });
    const uint64_t good = ok / reps, total = bytes / reps;
    printf("{\"n\": %llu, \"threads\": %d, \"reps\": %d, \"parse_ms\": %.3f, \"parse_per_s\": %.0f, \"parse_ok\": %llu, "
           "\"format_ms\": %.3f, \"format_per_s\": %.0f, \"format_bytes\": %llu}\n",
           (unsigned long long)n, T, reps, parse_ms, n / parse_ms * 1e3, (unsigned long long)good, format_ms,
           n / format_ms * 1e3, (unsigned long long)total);
    return 0;
}
