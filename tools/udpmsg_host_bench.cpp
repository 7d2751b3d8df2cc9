// udpmsg_host_bench.cpp -- the scalar host ABI of include/hyobfs_udpmsg.h on T threads:
// what the same work costs without a GPU, next to scripts/bench_udpmsg.py's device legs.
//
// N messages with bimodal data (40 % 64 B / 60 % 1350 B, SplitMix64), one 11-byte
// address, max_size 1200, split evenly over T threads.  Each thread owns its slice of the
// input and an output buffer of exactly the bytes its slice needs, and runs
//   send   hyobfs_udp_send_frags per message (sendMessageAutoFrag: header + payload copy)
//   parse  hyobfs_udp_parse per datagram that leg produced
// REPS times each; the time of a leg is the median over the repetitions of the wall time
// from a common start until the last thread is done.  Prints one JSON line.
//
//   g++ -O2 -std=c++17 tools/udpmsg_host_bench.cpp -o tools/udpmsg_host_bench -ldl -lpthread
//   tools/udpmsg_host_bench hysteria_amd/libhyobfs.so [N = 1048576] [T = 16] [REPS = 5]
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/hyobfs_udpmsg.h"

static uint64_t sm64_at(uint64_t seed, uint64_t k) {
    uint64_t z = seed + (k + 1) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

typedef int (*send_fn)(const hyobfs_udp_meta*, const uint8_t*, const uint8_t*, uint32_t, uint8_t*, size_t, uint32_t*,
                       uint32_t*);
typedef int (*parse_fn)(const uint8_t*, size_t, hyobfs_udp_parsed*);

struct Slice {
    std::vector<uint32_t> len;
    std::vector<uint8_t> data, out;
    std::vector<uint32_t> dgram_len;   // of the last send leg
    uint64_t payload = 0, parsed_ok = 0;
};

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s LIBHYOBFS [N] [T] [REPS]\n", argv[0]);
        return 2;
    }
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) {
        fprintf(stderr, "%s\n", dlerror());
        return 2;
    }
    const send_fn send = (send_fn)dlsym(lib, "hyobfs_udp_send_frags");
    const parse_fn parse = (parse_fn)dlsym(lib, "hyobfs_udp_parse");
    if (!send || !parse) return 2;
    const uint64_t n = argc > 2 ? strtoull(argv[2], nullptr, 10) : (1ull << 20);
    const int T = argc > 3 ? atoi(argv[3]) : 16, reps = argc > 4 ? atoi(argv[4]) : 5;
    static const uint8_t addr[] = "10.0.0.1:53";
    const uint32_t hdr = 20;   // HeaderSize: 8 + 1 + 11
    std::vector<Slice> S(T);
    uint64_t payload = 0, out_bytes = 0, dgrams = 0;
    for (int t = 0; t < T; ++t) {
        const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
        uint64_t need = 0;
        for (uint64_t i = lo; i < hi; ++i) {
            const uint32_t L = sm64_at(3, i) % 10 < 4 ? 64u : 1350u;
            S[t].len.push_back(L);
            S[t].payload += L;
            const uint32_t frags = hdr + L <= 1200 ? 1 : (L + 1179) / 1180;
            need += (uint64_t)frags * hdr + L;
            dgrams += frags;
        }
        S[t].data.resize(S[t].payload);
        for (uint64_t k = 0; k + 8 <= S[t].data.size(); k += 8) {
            const uint64_t v = sm64_at(6 + t, k);
            memcpy(&S[t].data[k], &v, 8);
        }
        S[t].out.resize(need);
        payload += S[t].payload;
        out_bytes += need;
    }
    auto run = [&](bool do_parse) {
        std::vector<double> ms;
        for (int r = 0; r < reps; ++r) {
            std::atomic<int> ready{0};
            std::atomic<bool> go{false};
            std::vector<std::thread> th;
            for (int t = 0; t < T; ++t)
                th.emplace_back([&, t] {
                    Slice& s = S[t];
                    ready.fetch_add(1);
                    while (!go.load(std::memory_order_acquire)) {
                    }
                    if (!do_parse) {
                        s.dgram_len.clear();
                        uint64_t in_at = 0, out_at = 0;
                        uint32_t lens[HYOBFS_UDP_MAX_FRAGS], count;
                        for (size_t i = 0; i < s.len.size(); ++i) {
                            const hyobfs_udp_meta m{(uint32_t)i, (uint16_t)(1 + i % 65535), 0, 1200, 11, 0};
                            if (send(&m, addr, s.data.data() + in_at, s.len[i], s.out.data() + out_at, s.out.size() - out_at,
                                     lens, &count) != HYOBFS_OK)
                                abort();
                            for (uint32_t k = 0; k < count; ++k) {
                                s.dgram_len.push_back(lens[k]);
                                out_at += lens[k];
                            }
                            in_at += s.len[i];
                        }
                    } else {
                        uint64_t at = 0, ok = 0;
                        hyobfs_udp_parsed p;
                        for (uint32_t L : s.dgram_len) {
                            ok += parse(s.out.data() + at, L, &p) == HYOBFS_OK;
                            at += L;
                        }
                        s.parsed_ok = ok;
                    }
                });
            while (ready.load() < T) {
            }
            const auto t0 = std::chrono::steady_clock::now();
            go.store(true, std::memory_order_release);
            for (auto& x : th) x.join();
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        return ms[ms.size() / 2];
    };
    const double send_ms = run(false), parse_ms = run(true);
    uint64_t ok = 0;
    for (auto& s : S) ok += s.parsed_ok;
    if (ok != dgrams) {
        fprintf(stderr, "parsed %llu of %llu datagrams\n", (unsigned long long)ok, (unsigned long long)dgrams);
        return 1;
    }
    printf("{\"n\": %llu, \"threads\": %d, \"reps\": %d, \"datagrams\": %llu, \"payload_bytes\": %llu, \"datagram_bytes\": %llu, "
           "\"send\": {\"ms\": %.3f, \"msgs_per_s\": %.0f, \"payload_GiB_per_s\": %.2f}, "
           "\"parse\": {\"ms\": %.3f, \"datagrams_per_s\": %.0f}}\n",
           (unsigned long long)n, T, reps, (unsigned long long)dgrams, (unsigned long long)payload,
           (unsigned long long)out_bytes, send_ms, n / send_ms * 1e3, payload / send_ms * 1e3 / 1073741824.0, parse_ms,
           dgrams / parse_ms * 1e3);
    return 0;
}
