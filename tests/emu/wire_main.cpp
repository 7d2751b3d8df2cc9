// wire_main.cpp -- stand-alone driver of the realm punch matcher and the Gecko
// parse and encode kernels on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_wire_cases.py compiles this file under
// AddressSanitizer, links it against tests/emu/libhyobfs_emu.so (the kernel
// sources built for the host against hip_emu.h) and runs it as a child process:
// a program with its own main, nothing is preloaded.
//
//   wire_main CASES
// CASES (tests/wire_cases.py writes it) is a run of sections, all little-endian,
// each opening with a u32 tag:
//   1 punch:  u32 m, null_out; u64 n, buf_len, total; m x 48 attempt bytes;
//             total x u64 in_off; total x u32 in_len; total x u8 real; buf.
//             The first n entries are matched (m == 0: `attempts` null; null_out:
//             `type` and `padding` null).  Every byte of buf outside the `real`
//             entries is poisoned.  Prints one line per entry: match type padding.
//   2 parse:  u64 n, buf_len; n x u64 in_off; n x u32 in_len; buf; n x 16 bytes
//             of expected records.  Every byte of buf outside the datagrams is
//             poisoned.
//   3 encode: u32 psk_len; psk; u64 n, msg_len; pad key (32), nonce (12); n x 16
//             frame bytes; n x u64 salts; n x u64 out_off; msg; u64 out_len; the
//             expected out (every byte no frame covers holds the sentinel 0xA5).
//   4 far:    as 3 up to msg, then u64 lo, map_len, n_windows and per window u64
//             start, len and the expected bytes.  `out` is a sparse anonymous
//             mapping standing for out[lo, lo + map_len): only the windows are
//             filled with the sentinel before the call and compared after it.
// Every array lies in an allocation of exactly its size, so AddressSanitizer stops
// the program at the first byte read or written past the API's promise.  Sections
// 2-4 print `<kind> ... bad=<mismatching records or bytes> first=<position>`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <sanitizer/asan_interface.h>
#include <sys/mman.h>

#include "../../include/hyobfs_gecko.h"
#include "../../include/hyobfs_realm.h"

static FILE* g_f;
static const uint8_t kSentinel = 0xA5;

static void rd(void* p, size_t n) {
    if (n && fread(p, 1, n, g_f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
}
static uint32_t rd32() {
    uint32_t v;
    rd(&v, 4);
    return v;
}
static uint64_t rd64() {
    uint64_t v;
    rd(&v, 8);
    return v;
}
// n elements in an allocation of exactly n * sizeof(T) bytes, read from the file
template <class T>
static std::unique_ptr<T[]> exact(uint64_t n) {
    std::unique_ptr<T[]> p(static_cast<T*>(operator new[](n * sizeof(T) ? n * sizeof(T) : 1)));
    rd(p.get(), n * sizeof(T));
    return p;
}
// poisons every byte of buf[0, len) that no [off, off + n) range covers
static void poison_gaps(uint8_t* buf, uint64_t len, const std::vector<std::pair<uint64_t, uint64_t>>& used) {
    std::vector<uint8_t> cov(len, 0);
    for (auto& u : used)
        if (u.first + u.second <= len) memset(cov.data() + u.first, 1, u.second);
    for (uint64_t a = 0; a < len;) {
        if (cov[a]) {
            ++a;
            continue;
        }
        uint64_t b = a;
        while (b < len && !cov[b]) ++b;
        ASAN_POISON_MEMORY_REGION(buf + a, b - a);
        a = b;
    }
}

static int run_punch() {
    const uint32_t m = rd32(), null_out = rd32();
    const uint64_t n = rd64(), buf_len = rd64(), total = rd64();
    auto att = exact<hyobfs_punch_attempt>(m);
    auto off_all = exact<uint64_t>(total);
    auto len_all = exact<uint32_t>(total);
    auto real = exact<uint8_t>(total);
    auto buf = exact<uint8_t>(buf_len);
    std::unique_ptr<uint64_t[]> off(new uint64_t[n ? n : 1]);
    std::unique_ptr<uint32_t[]> len(new uint32_t[n ? n : 1]);
    memcpy(off.get(), off_all.get(), n * 8);
    memcpy(len.get(), len_all.get(), n * 4);
    std::vector<std::pair<uint64_t, uint64_t>> used;
    for (uint64_t i = 0; i < total; ++i)
        if (real[i]) used.push_back({off_all[i], len_all[i]});
    poison_gaps(buf.get(), buf_len, used);
    std::unique_ptr<int32_t[]> match(new int32_t[n ? n : 1]);
    std::unique_ptr<uint8_t[]> type(new uint8_t[n ? n : 1]);
    std::unique_ptr<uint32_t[]> padding(new uint32_t[n ? n : 1]);
    memset(match.get(), 0xEE, n * 4);
    memset(type.get(), 0xEE, n);
    memset(padding.get(), 0xEE, n * 4);
    const int st = hyobfs_punch_match_batch(buf.get(), off.get(), len.get(), n, m ? att.get() : nullptr, m, match.get(),
                                            null_out ? nullptr : type.get(), null_out ? nullptr : padding.get(), nullptr);
    ASAN_UNPOISON_MEMORY_REGION(buf.get(), buf_len);
    if (st != HYOBFS_OK) {
        fprintf(stderr, "punch_match_batch failed: %d\n", st);
        return 3;
    }
    printf("punch n=%llu m=%u\n", (unsigned long long)n, m);
    for (uint64_t i = 0; i < n; ++i) printf("%d %u %u\n", match[i], type[i], padding[i]);
    return 0;
}

static int run_parse() {
    const uint64_t n = rd64(), buf_len = rd64();
    auto off = exact<uint64_t>(n);
    auto len = exact<uint32_t>(n);
    auto buf = exact<uint8_t>(buf_len);
    auto exp = exact<hyobfs_gecko_parsed>(n);
    std::vector<std::pair<uint64_t, uint64_t>> used;
    for (uint64_t i = 0; i < n; ++i) used.push_back({off[i], len[i]});
    poison_gaps(buf.get(), buf_len, used);
    std::unique_ptr<hyobfs_gecko_parsed[]> got(new hyobfs_gecko_parsed[n ? n : 1]);
    memset(got.get(), 0xEE, n * sizeof(hyobfs_gecko_parsed));
    const int st = hyobfs_gecko_parse_batch(buf.get(), off.get(), len.get(), n, got.get(), nullptr);
    ASAN_UNPOISON_MEMORY_REGION(buf.get(), buf_len);
    if (st != HYOBFS_OK) {
        fprintf(stderr, "gecko_parse_batch failed: %d\n", st);
        return 3;
    }
    uint64_t bad = 0;
    long long first = -1;
    for (uint64_t i = 0; i < n; ++i)
        if (memcmp(&got[i], &exp[i], sizeof(hyobfs_gecko_parsed)) != 0 && bad++ == 0) first = (long long)i;
    printf("parse n=%llu bad=%llu first=%lld", (unsigned long long)n, (unsigned long long)bad, first);
    if (first >= 0) {
        const hyobfs_gecko_parsed &g = got[first], &e = exp[first];
        printf(" len=%u got=%d,%u,%u,%u,%u,%u exp=%d,%u,%u,%u,%u,%u", len[first], g.status, g.pad_len, g.msg_id,
               g.idx_total, g.payload_off, g.payload_len, e.status, e.pad_len, e.msg_id, e.idx_total, e.payload_off,
               e.payload_len);
    }
    printf("\n");
    return 0;
}

// sections 3 and 4
static int run_encode(bool far) {
    const uint32_t psk_len = rd32();
    auto psk = exact<uint8_t>(psk_len);
    hyobfs_gecko_batch b;
    memset(&b, 0, sizeof b);
    b.n = rd64();
    const uint64_t msg_len = rd64();
    rd(b.pad_key, 32);
    rd(b.pad_nonce, 12);
    auto frames = exact<hyobfs_gecko_frame>(b.n);
    auto salts = exact<uint64_t>(b.n);
    auto off = exact<uint64_t>(b.n);
    auto msg = exact<uint8_t>(msg_len);
    b.msg = msg.get();
    b.frames = frames.get();
    b.salts = salts.get();
    b.out_off = off.get();
    hyobfs_salamander* ctx = nullptr;
    if (hyobfs_salamander_new(psk.get(), psk_len, 0, &ctx) != HYOBFS_OK) {
        fprintf(stderr, "salamander_new failed\n");
        return 3;
    }
    uint64_t bad = 0, compared = 0;
    long long first = -1;
    int st;
    if (!far) {
        const uint64_t out_len = rd64();
        auto exp = exact<uint8_t>(out_len);
        std::unique_ptr<uint8_t[]> out(new uint8_t[out_len ? out_len : 1]);
        memset(out.get(), kSentinel, out_len);
        b.out = out.get();
        st = hyobfs_gecko_encode_batch(ctx, &b, nullptr);
        for (uint64_t i = 0; i < out_len; ++i)
            if (out[i] != exp[i] && bad++ == 0) first = (long long)i;
        printf("encode n=%llu out=%llu", (unsigned long long)b.n, (unsigned long long)out_len);
    } else {
        const uint64_t lo = rd64(), map_len = rd64(), nwin = rd64();
        uint8_t* map = static_cast<uint8_t*>(
            mmap(nullptr, map_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0));
        if (map == MAP_FAILED) {
            fprintf(stderr, "mmap of %llu bytes failed\n", (unsigned long long)map_len);
            return 3;
        }
        std::vector<uint64_t> start(nwin);
        std::vector<std::vector<uint8_t>> exp(nwin);
        for (uint64_t w = 0; w < nwin; ++w) {
            start[w] = rd64();
            exp[w].resize(rd64());
            rd(exp[w].data(), exp[w].size());
            if (start[w] < lo || start[w] + exp[w].size() > lo + map_len) return 2;
            memset(map + (start[w] - lo), kSentinel, exp[w].size());
        }
        b.out = map - lo;   // out[lo, lo + map_len) is the mapping
        st = hyobfs_gecko_encode_batch(ctx, &b, nullptr);
        for (uint64_t w = 0; w < nwin; ++w)
            for (uint64_t i = 0; i < exp[w].size(); ++i, ++compared)
                if (map[start[w] - lo + i] != exp[w][i] && bad++ == 0) first = (long long)(start[w] + i);
        munmap(map, map_len);
        printf("far n=%llu windows=%llu bytes=%llu", (unsigned long long)b.n, (unsigned long long)nwin,
               (unsigned long long)compared);
    }
    hyobfs_salamander_free(ctx);
    if (st != HYOBFS_OK) {
        fprintf(stderr, "gecko_encode_batch failed: %d\n", st);
        return 3;
    }
    printf(" bad=%llu first=%lld\n", (unsigned long long)bad, first);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    g_f = fopen(argv[1], "rb");
    if (!g_f) return 2;
    uint32_t tag;
    while (fread(&tag, 1, 4, g_f) == 4) {
        const int rc = tag == 1 ? run_punch() : tag == 2 ? run_parse() : tag == 3 ? run_encode(false)
                       : tag == 4                                                ? run_encode(true)
                                                                                 : 2;
        if (rc) return rc;
    }
    fclose(g_f);
    printf("done\n");
    return 0;
}
