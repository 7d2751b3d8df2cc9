// addr_main.cpp -- stand-alone driver of the request-address kernels on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_addr.py compiles this file together with
// hysteria_amd/csrc/addr.hip and udpmsg.hip for the host against hip_emu.h
// (-DHYOBFS_EMULATE) under AddressSanitizer and runs it as a child process.
//
//   addr_main CASES RESULTS
// CASES (tests/addr_cases.py writes it, little-endian) is a sequence of operations,
// each starting with a u32 kind:
//   1 parse_batch      u32 n, u32 buf_len, the buffer, u64 off[n], u32 len[n]
//   2 parse_udp_batch  the same, the items being relay datagrams: they are parsed by
//                      hyobfs_udp_parse_batch first
//   3 format_batch     u32 n, u32 stride, u32 mis, u32 with_meta, u64 base_off,
//                      n x (16 bytes ip, u8 family, u16 port)
// The input buffer of 1 / 2 is an allocation of exactly its size, poisoned as a whole;
// then every item of at most 2048 bytes is made addressable again (to the sanitizer's
// 8-byte granularity), so a read between the items, or of an item that is too long,
// stops the program.  Every output array lies between 64 guard bytes (0xA5, and
// poisoned for the sanitizer) in an allocation of its own, is pre-filled with 0xA5
// too, and is reported with its guards.  For 1 / 2 the ipv4 and ipv6 arrays start
// (number of items mod 4) bytes into their payload; for 3 the ip input and the output
// rows start `mis` bytes in.
// RESULTS, per operation:
//   1  i32 rc, then status, name_off, name_len, ipv4, ipv6, ip_flags, port
//   2  i32 rc of the message parse, i32 rc, then the same arrays
//   3  i32 rc, then status, out_len, meta (with_meta only), out
// each array as 64 guard bytes, `mis` bytes, the payload, 64 guard bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs_addr.h"

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

constexpr size_t kGuard = 64;

// `bytes` payload bytes, `mis` bytes into the space between two guards; everything 0xA5
struct Guarded {
    std::unique_ptr<uint8_t[]> mem;
    size_t mis, bytes;
    Guarded(size_t bytes_, size_t mis_ = 0) : mem(new uint8_t[2 * kGuard + mis_ + bytes_]), mis(mis_), bytes(bytes_) {
        memset(mem.get(), 0xA5, 2 * kGuard + mis + bytes);
        ASAN_POISON_MEMORY_REGION(mem.get(), kGuard + mis);
        ASAN_POISON_MEMORY_REGION(mem.get() + kGuard + mis + bytes, kGuard);
    }
    template <class T>
    T* ptr() { return reinterpret_cast<T*>(mem.get() + kGuard + mis); }
    void dump() {
        ASAN_UNPOISON_MEMORY_REGION(mem.get(), 2 * kGuard + mis + bytes);
        wr(mem.get(), 2 * kGuard + mis + bytes);
    }
};

static void op_parse(bool udp) {
    const uint32_t n = rd32(), buf_len = rd32();
    std::unique_ptr<uint8_t[]> buf(new uint8_t[buf_len ? buf_len : 1]);
    need(buf.get(), buf_len);
    std::unique_ptr<uint64_t[]> off(new uint64_t[n ? n : 1]);
    std::unique_ptr<uint32_t[]> len(new uint32_t[n ? n : 1]);
    need(off.get(), 8 * (size_t)n);
    need(len.get(), 4 * (size_t)n);
    ASAN_POISON_MEMORY_REGION(buf.get(), buf_len);
    for (uint32_t i = 0; i < n; ++i)
        if (len[i] && (udp || len[i] <= HYOBFS_UDP_MAX_ADDR)) ASAN_UNPOISON_MEMORY_REGION(buf.get() + off[i], len[i]);
    const size_t mis = n % 4;
    Guarded status(4 * (size_t)n), name_off(8 * (size_t)n), name_len(4 * (size_t)n), ipv4(4 * (size_t)n, mis),
        ipv6(16 * (size_t)n, mis), ip_flags(n), port(2 * (size_t)n);
    int32_t rc0 = 0, rc;
    if (udp) {
        std::unique_ptr<hyobfs_udp_parsed[]> parsed(new hyobfs_udp_parsed[n ? n : 1]);
        rc0 = hyobfs_udp_parse_batch(buf.get(), off.get(), len.get(), n, parsed.get(), nullptr);
        rc = hyobfs_addr_parse_udp_batch(buf.get(), off.get(), parsed.get(), n, status.ptr<int32_t>(), name_off.ptr<uint64_t>(),
                                         name_len.ptr<uint32_t>(), ipv4.ptr<uint8_t>(), ipv6.ptr<uint8_t>(),
                                         ip_flags.ptr<uint8_t>(), port.ptr<uint16_t>(), nullptr);
        wr(&rc0, 4);
    } else {
        rc = hyobfs_addr_parse_batch(buf.get(), off.get(), len.get(), n, status.ptr<int32_t>(), name_off.ptr<uint64_t>(),
                                     name_len.ptr<uint32_t>(), ipv4.ptr<uint8_t>(), ipv6.ptr<uint8_t>(),
                                     ip_flags.ptr<uint8_t>(), port.ptr<uint16_t>(), nullptr);
    }
    ASAN_UNPOISON_MEMORY_REGION(buf.get(), buf_len);
    wr(&rc, 4);
    for (Guarded* g : {&status, &name_off, &name_len, &ipv4, &ipv6, &ip_flags, &port}) g->dump();
}

static void op_format() {
    const uint32_t n = rd32(), stride = rd32(), mis = rd32(), with_meta = rd32();
    const uint64_t base_off = rd64();
    std::unique_ptr<uint8_t[]> ip(new uint8_t[16 * (size_t)n + mis]);   // exactly what is read, `mis` bytes in
    std::unique_ptr<uint8_t[]> family(new uint8_t[n ? n : 1]);
    std::unique_ptr<uint16_t[]> port(new uint16_t[n ? n : 1]);
    for (uint32_t i = 0; i < n; ++i) {
        need(ip.get() + mis + 16 * (size_t)i, 16);
        need(&family[i], 1);
        need(&port[i], 2);
    }
    Guarded status(4 * (size_t)n), out_len(4 * (size_t)n), meta(sizeof(hyobfs_udp_meta) * (size_t)n),
        out((size_t)n * stride, mis);
    const int32_t rc = hyobfs_addr_format_batch(ip.get() + mis, family.get(), port.get(), n, out.ptr<uint8_t>(), stride, base_off,
                                                out_len.ptr<uint32_t>(), with_meta ? meta.ptr<hyobfs_udp_meta>() : nullptr,
                                                status.ptr<int32_t>(), nullptr);
    wr(&rc, 4);
    status.dump();
    out_len.dump();
    if (with_meta) meta.dump();
    out.dump();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    g_f = fopen(argv[1], "rb");
    g_o = fopen(argv[2], "wb");
    if (!g_f || !g_o) return 2;
    uint32_t kind;
    while (rd(&kind, 4)) {
        if (kind == 1 || kind == 2)
            op_parse(kind == 2);
        else if (kind == 3)
            op_format();
        else
            return 2;
    }
    fclose(g_f);
    if (fclose(g_o) != 0) return 2;
    printf("done\n");
    return 0;
}
