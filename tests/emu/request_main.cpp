// request_main.cpp -- stand-alone driver of the request-hook kernels on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_request.py compiles this file together with
// hysteria_amd/csrc/request.hip, request_host.cpp, addr.hip and addr_host.cpp for
// the host against hip_emu.h (-DHYOBFS_EMULATE) under AddressSanitizer
// and UndefinedBehaviorSanitizer and runs it as a child process.
//
//   request_main CASES RESULTS
// CASES (tests/request_cases.py writes it, little-endian) is a sequence of operations,
// each starting with a u32 kind:
//   1 request parse  u32 n, u32 buf_len, the buffer, u64 off[n], u32 len[n]
//   2 check          u32 n, u32 buf_len, u32 is_udp, u32 rewrite_domain, i32 n_ranges (-1: no
//                    port set), u32 with_gate, the buffer, off, len, i32 gate[n] (with_gate
//                    only), n_ranges x (u16 start, u16 end)
//   3 rewrite        u32 n, u32 buf_len, u32 name_stride, u32 out_stride, u32 mis, u32
//                    with_gate, u64 base_off, the buffer, off, len, gate (with_gate only),
//                    u8 check[n], n sniff results, n name rows, u32 name_reads[n]
//   4 response       u32 n, u32 n_msgs, u32 out_stride, u32 mis, u64 seed, u32 msgs_len, the
//                    messages' buffer, u64 msg_off[n_msgs], u32 msg_len[n_msgs], u8 ok[n],
//                    u32 msg_idx[n], u32 pad_len[n]
// Every input buffer is an allocation of exactly its size, poisoned as a whole; then only
// what the call may read is made addressable again (to the sanitizer's 8-byte
// granularity): the items whose gate is open (for 2, those of at most 2048 bytes), the
// first name_reads[i] bytes of name row i, the messages.  Every output array lies between
// 64 guard bytes (0xA5, and poisoned) in an allocation of its own, is pre-filled with 0xA5
// too, and is reported with its guards; the rows of 3 and 4 start `mis` bytes in.
// RESULTS, per operation: i32 rc (2: the port set's rc first), then
//   1  status, need, addr_off, addr_len, rest_off, rest_len
//   2  check
//   3  status, out_len, rewritten, row_off, out
//   4  status, out_len, out
// each array as 64 guard bytes, `mis` bytes, the payload, 64 guard bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs_request.h"

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

// an input of exactly n bytes (n elements of T), read from the case file
template <class T>
struct Input {
    std::unique_ptr<T[]> mem;
    size_t n;
    explicit Input(size_t n_) : mem(new T[n_ ? n_ : 1]), n(n_) { need(mem.get(), sizeof(T) * n); }
    T* get() { return mem.get(); }
    T& operator[](size_t i) { return mem[i]; }
    void poison() { ASAN_POISON_MEMORY_REGION(mem.get(), sizeof(T) * n); }
    void unpoison() { ASAN_UNPOISON_MEMORY_REGION(mem.get(), sizeof(T) * n); }
};

static void op_parse() {
    const uint32_t n = rd32(), buf_len = rd32();
    Input<uint8_t> buf(buf_len);
    Input<uint64_t> off(n);
    Input<uint32_t> len(n);
    buf.poison();
    for (uint32_t i = 0; i < n; ++i)
        if (len[i]) ASAN_UNPOISON_MEMORY_REGION(buf.get() + off[i], len[i]);
    Guarded status(4 * (size_t)n), need_(4 * (size_t)n), addr_off(8 * (size_t)n), addr_len(4 * (size_t)n),
        rest_off(8 * (size_t)n), rest_len(4 * (size_t)n);
    const int32_t rc = hyobfs_tcp_request_parse_batch(buf.get(), off.get(), len.get(), n, status.ptr<int32_t>(),
                                                      need_.ptr<uint32_t>(), addr_off.ptr<uint64_t>(), addr_len.ptr<uint32_t>(),
                                                      rest_off.ptr<uint64_t>(), rest_len.ptr<uint32_t>(), nullptr);
    buf.unpoison();
    wr(&rc, 4);
    for (Guarded* g : {&status, &need_, &addr_off, &addr_len, &rest_off, &rest_len}) g->dump();
}

static void op_check() {
    const uint32_t n = rd32(), buf_len = rd32(), is_udp = rd32(), rewrite_domain = rd32();
    const int32_t n_ranges = (int32_t)rd32();
    const uint32_t with_gate = rd32();
    Input<uint8_t> buf(buf_len);
    Input<uint64_t> off(n);
    Input<uint32_t> len(n);
    Input<int32_t> gate(with_gate ? n : 0);
    Input<hyobfs_port_range> ranges(n_ranges > 0 ? (size_t)n_ranges : 0);
    buf.poison();
    for (uint32_t i = 0; i < n; ++i)
        if (len[i] && len[i] <= HYOBFS_REQ_MAX_ADDR && !(with_gate && gate[i])) ASAN_UNPOISON_MEMORY_REGION(buf.get() + off[i], len[i]);
    hyobfs_portset* set = nullptr;
    const int32_t rc0 = n_ranges < 0 ? 0 : hyobfs_portset_new(ranges.get(), (uint32_t)n_ranges, 0, &set);
    Guarded check(n);
    const int32_t rc = hyobfs_sniff_check_batch(buf.get(), off.get(), len.get(), with_gate ? gate.get() : nullptr, n, (int)is_udp,
                                                (int)rewrite_domain, set, check.ptr<uint8_t>(), nullptr);
    hyobfs_portset_free(set);
    buf.unpoison();
    wr(&rc0, 4);
    wr(&rc, 4);
    check.dump();
}

static void op_rewrite() {
    const uint32_t n = rd32(), buf_len = rd32(), name_stride = rd32(), stride = rd32(), mis = rd32(), with_gate = rd32();
    const uint64_t base_off = rd64();
    Input<uint8_t> buf(buf_len);
    Input<uint64_t> off(n);
    Input<uint32_t> len(n);
    Input<int32_t> gate(with_gate ? n : 0);
    Input<uint8_t> check(n);
    Input<hyobfs_sniff_result> sres(n);
    Input<uint8_t> names((size_t)n * name_stride);
    Input<uint32_t> reads(n);
    buf.poison();
    names.poison();
    for (uint32_t i = 0; i < n; ++i) {
        if (len[i] && !(with_gate && gate[i])) ASAN_UNPOISON_MEMORY_REGION(buf.get() + off[i], len[i]);
        if (reads[i]) ASAN_UNPOISON_MEMORY_REGION(names.get() + (size_t)i * name_stride, reads[i]);
    }
    Guarded status(4 * (size_t)n), out_len(4 * (size_t)n), rewritten(n), row_off(8 * (size_t)n), out((size_t)n * stride, mis);
    const int32_t rc = hyobfs_request_rewrite_batch(buf.get(), off.get(), len.get(), with_gate ? gate.get() : nullptr, check.get(),
                                                    names.get(), name_stride, sres.get(), n, out.ptr<uint8_t>(), stride, base_off,
                                                    row_off.ptr<uint64_t>(), out_len.ptr<uint32_t>(), rewritten.ptr<uint8_t>(),
                                                    status.ptr<int32_t>(), nullptr);
    buf.unpoison();
    names.unpoison();
    wr(&rc, 4);
    for (Guarded* g : {&status, &out_len, &rewritten, &row_off, &out}) g->dump();
}

static void op_response() {
    const uint32_t n = rd32(), n_msgs = rd32(), stride = rd32(), mis = rd32();
    const uint64_t seed = rd64();
    const uint32_t msgs_len = rd32();
    Input<uint8_t> msgs(msgs_len);
    Input<uint64_t> msg_off(n_msgs);
    Input<uint32_t> msg_len(n_msgs);
    Input<uint8_t> ok(n);
    Input<uint32_t> msg_idx(n), pad_len(n);
    msgs.poison();
    for (uint32_t m = 0; m < n_msgs; ++m)
        if (msg_len[m]) ASAN_UNPOISON_MEMORY_REGION(msgs.get() + msg_off[m], msg_len[m]);
    Guarded status(4 * (size_t)n), out_len(4 * (size_t)n), out((size_t)n * stride, mis);
    const int32_t rc = hyobfs_tcp_response_build_batch(ok.get(), msg_idx.get(), msgs.get(), msg_off.get(), msg_len.get(), n_msgs,
                                                       pad_len.get(), seed, n, out.ptr<uint8_t>(), stride, out_len.ptr<uint32_t>(),
                                                       status.ptr<int32_t>(), nullptr);
    msgs.unpoison();
    wr(&rc, 4);
    for (Guarded* g : {&status, &out_len, &out}) g->dump();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    g_f = fopen(argv[1], "rb");
    g_o = fopen(argv[2], "wb");
    if (!g_f || !g_o) return 2;
    uint32_t kind;
    while (rd(&kind, 4)) {
        if (kind == 1)
            op_parse();
        else if (kind == 2)
            op_check();
        else if (kind == 3)
            op_rewrite();
        else if (kind == 4)
            op_response();
        else
            return 2;
    }
    fclose(g_f);
    if (fclose(g_o) != 0) return 2;
    printf("done\n");
    return 0;
}
