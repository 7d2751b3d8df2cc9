// gecko_rx_main.cpp -- stand-alone driver of Gecko's device receive path on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_gecko_rx.py compiles this file under
// AddressSanitizer, links it against the emulated library (tests/emu/libhyobfs_emu.so)
// and runs it as a child process.
//
//   gecko_rx_main CASES RESULTS
// CASES (tests/gecko_rx_cases.py writes it, little-endian) is a sequence of operations,
// each starting with a u32 kind:
//   1 peek   u32 psk_len, the PSK, u64 buf_len, u32 n, u64 off[n], u32 wire_len[n], then
//            the datagrams back to back (wire_len[i] bytes each)
//   2 open   u64 buf_len, u32 n, u32 n_idx, u32 m, u64 off[n], u32 wire_len[n] (as the
//            call is told), u32 real_len[n] (the bytes that follow), 16-byte records [n],
//            32-byte keys [n], u32 chunk_idx[n_idx], u64 msg_first[m + 1], u32 out_cap[m],
//            u32 gap[m] (guard bytes in front of message j's output), then the datagrams
// The datagrams sit at their offsets in one buffer of exactly buf_len bytes; every byte
// of it that belongs to no datagram is poisoned as far as the sanitizer's 8-byte
// granules allow (8-aligned slots: every byte between two datagrams).  Every other array
// sits in an allocation of exactly its size.  Outputs are pre-filled with 0xA5; the open
// output is the gaps and capacities one after the other plus 16 trailing guard bytes.
// RESULTS, per operation:
//   1  i32 rc, n records, n keys
//   2  i32 rc, i32 status[m], u32 out_len[m], u64 bytes, the output buffer
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs_gecko.h"

static FILE *g_f, *g_o;

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, g_f) == n; }
static void need(void* p, size_t n) {
    if (!rd(p, n)) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
}
static uint32_t rd32() {
    uint32_t v;
    need(&v, 4);
    return v;
}
static uint64_t rd64() {
    uint64_t v;
    need(&v, 8);
    return v;
}
static void wr(const void* p, size_t n) {
    if (n && fwrite(p, 1, n, g_o) != n) exit(2);
}
template <class T>
static std::unique_ptr<T[]> exact(size_t n) {   // exactly n items, read from the case file
    std::unique_ptr<T[]> p(new T[n]);
    need(p.get(), n * sizeof(T));
    return p;
}
template <class T>
static std::unique_ptr<T[]> filled(size_t n) {   // exactly n items, every byte 0xA5
    std::unique_ptr<T[]> p(new T[n]);
    memset(static_cast<void*>(p.get()), 0xA5, n * sizeof(T));
    return p;
}

// exactly n bytes at a 16-aligned address (the residues of the cases are then those of the addresses)
struct Bytes {
    uint8_t* p = nullptr;
    Bytes(size_t n, int fill) {
        if (posix_memalign(reinterpret_cast<void**>(&p), 16, n ? n : 1) != 0) exit(2);
        memset(p, fill, n);
    }
    ~Bytes() { free(p); }
    Bytes(const Bytes&) = delete;
    uint8_t* get() const { return p; }
};

// the wire buffer: datagram i's real[i] bytes at off[i], everything else poisoned
struct Wire {
    Bytes buf;
    uint64_t len;
    Wire(uint64_t buf_len, size_t n, const uint64_t* off, const uint32_t* real) : buf(buf_len, 0xEE), len(buf_len) {
        for (size_t i = 0; i < n; ++i) need(buf.get() + off[i], real[i]);
        std::vector<size_t> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return off[a] < off[b]; });
        uint64_t cur = 0;
        for (size_t i : order) {
            poison(cur, off[i]);
            cur = std::max(cur, off[i] + real[i]);
        }
    }
    void poison(uint64_t a, uint64_t b) {   // [a, b): up to the last granule boundary (the allocation is 16-aligned)
        b &= ~7ull;
        if (b > a) ASAN_POISON_MEMORY_REGION(buf.get() + a, b - a);
    }
    ~Wire() { ASAN_UNPOISON_MEMORY_REGION(buf.get(), len); }
};

static void op_peek() {
    const uint32_t psk_len = rd32();
    auto psk = exact<uint8_t>(psk_len);
    const uint64_t buf_len = rd64();
    const uint32_t n = rd32();
    auto off = exact<uint64_t>(n);
    auto wlen = exact<uint32_t>(n);
    Wire w(buf_len, n, off.get(), wlen.get());
    hyobfs_salamander* ctx = nullptr;
    if (hyobfs_salamander_new(psk.get(), psk_len, 0, &ctx) != HYOBFS_OK) exit(3);
    auto parsed = filled<hyobfs_gecko_parsed>(n);
    auto keys = filled<uint8_t>(32 * (size_t)n);
    const int32_t rc = hyobfs_gecko_peek_batch(ctx, w.buf.get(), off.get(), wlen.get(), n, parsed.get(), keys.get(), nullptr);
    hyobfs_salamander_free(ctx);
    wr(&rc, 4);
    wr(parsed.get(), n * sizeof(hyobfs_gecko_parsed));
    wr(keys.get(), 32 * (size_t)n);
}

static void op_open() {
    const uint64_t buf_len = rd64();
    const uint32_t n = rd32(), n_idx = rd32(), m = rd32();
    auto off = exact<uint64_t>(n);
    auto wlen = exact<uint32_t>(n);
    auto real = exact<uint32_t>(n);
    auto parsed = exact<hyobfs_gecko_parsed>(n);
    auto keys = exact<uint8_t>(32 * (size_t)n);
    auto idx = exact<uint32_t>(n_idx);
    auto first = exact<uint64_t>((size_t)m + 1);
    auto cap = exact<uint32_t>(m);
    auto gap = exact<uint32_t>(m);
    Wire w(buf_len, n, off.get(), real.get());
    std::unique_ptr<uint64_t[]> out_off(new uint64_t[m]);
    uint64_t total = 0;
    for (uint32_t j = 0; j < m; ++j) {
        total += gap[j];
        out_off[j] = total;
        total += cap[j];
    }
    total += 16;
    Bytes out(total, 0xA5);
    auto out_len = filled<uint32_t>(m);
    auto status = filled<int32_t>(m);
    const int32_t rc = hyobfs_gecko_open_batch(w.buf.get(), off.get(), wlen.get(), parsed.get(), keys.get(), n, idx.get(),
                                               first.get(), m, out.get(), out_off.get(), cap.get(), out_len.get(),
                                               status.get(), nullptr);
    wr(&rc, 4);
    wr(status.get(), 4 * (size_t)m);
    wr(out_len.get(), 4 * (size_t)m);
    wr(&total, 8);
    wr(out.get(), total);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    g_f = fopen(argv[1], "rb");
    g_o = fopen(argv[2], "wb");
    if (!g_f || !g_o) return 2;
    uint32_t kind;
    while (rd(&kind, 4)) {
        if (kind == 1)
            op_peek();
        else if (kind == 2)
            op_open();
        else
            return 2;
    }
    fclose(g_f);
    if (fclose(g_o) != 0) return 2;
    printf("done\n");
    return 0;
}
