// udpmsg_main.cpp -- stand-alone driver of the UDP relay message kernels on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_udpmsg.py compiles this file together with
// hysteria_amd/csrc/udpmsg.hip for the host against hip_emu.h (-DHYOBFS_EMULATE)
// under AddressSanitizer and runs it as a child process.
//
//   udpmsg_main CASES RESULTS
// CASES (tests/udpmsg_cases.py writes it, little-endian) is a sequence of
// operations, each starting with a u32 kind:
//   1 frag_batch   u32 n, u64 out_cap, u64 dgram_cap, u32 out_mis, u32 spread, u32 addrs_len,
//                  the address bytes, n x (u32 session_id, packet_id, max_size,
//                  addr_len, u64 addr_off, u32 data_len), then the data of all
//                  messages back to back
//   2 parse_batch  u32 n, n x (u32 len, bytes)
//   3 assemble     the datagrams as for 2 (they are parsed first), u32 n_idx,
//                  the indices, u32 m, (m + 1) x u64 msg_first, m x (u32 out_cap,
//                  u32 gap in front of the message's output)
// Every input sits in an allocation of exactly its size; datagrams (2, 3) sit in
// 8-aligned slots of one buffer with the bytes between them poisoned.  For 1, spread = 0
// keeps the payloads back to back (every source residue mod 16) and the addresses as
// given (shared); spread = 1 gives every payload and every message's address a slot of
// its own (8-aligned) with the bytes up to the next slot poisoned, so a load that runs
// past one payload or address into its neighbour stops the program.  Every output
// array has exactly the stated length (a null pointer where that is 0) and is
// pre-filled with 0xA5.  The frag output buffer starts out_mis bytes into its
// allocation and ends with it; those leading bytes are reported with it.
// RESULTS, per operation:
//   1  i32 rc, status[n], u64 first[n + 1], totals[2], dgram_off[dgram_cap],
//      u32 dgram_len[dgram_cap], the out_mis + out_cap bytes of the allocation
//   2  i32 rc, n x hyobfs_udp_parsed
//   3  i32 rc of the parse, i32 rc, i32 status[m], u32 out_len[m], u64 bytes, the output buffer
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs_udpmsg.h"

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
static std::unique_ptr<T[]> filled(size_t n) {   // exactly n items (none: a null pointer), every byte 0xA5
    if (n == 0) return nullptr;
    std::unique_ptr<T[]> p(new T[n]);
    memset(p.get(), 0xA5, n * sizeof(T));
    return p;
}

// the datagrams in 8-aligned slots of one buffer, the gaps poisoned
struct Datagrams {
    std::vector<uint8_t> buf;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    void read() {
        const uint32_t n = rd32();
        std::vector<std::vector<uint8_t>> items(n);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; ++i) {
            len.push_back(rd32());
            items[i].resize(len[i]);
            need(items[i].data(), len[i]);
            off.push_back(total);
            total += (len[i] + 8) / 8 * 8;   // at least one poisoned byte after each
        }
        buf.assign(total + 8, 0xEE);
        for (uint32_t i = 0; i < n; ++i) {
            if (len[i]) memcpy(buf.data() + off[i], items[i].data(), len[i]);
            ASAN_POISON_MEMORY_REGION(buf.data() + off[i] + len[i], (len[i] + 8) / 8 * 8 - len[i]);
        }
    }
    ~Datagrams() { ASAN_UNPOISON_MEMORY_REGION(buf.data(), buf.size()); }
};

static void op_frag() {
    const uint32_t n = rd32();
    const uint64_t out_cap = rd64(), dgram_cap = rd64();
    const uint32_t mis = rd32(), spread = rd32(), addrs_len = rd32();
    std::unique_ptr<uint8_t[]> addrs(new uint8_t[addrs_len ? addrs_len : 1]);
    need(addrs.get(), addrs_len);
    std::unique_ptr<hyobfs_udp_meta[]> meta(new hyobfs_udp_meta[n]);
    std::unique_ptr<uint64_t[]> data_off(new uint64_t[n]);
    std::unique_ptr<uint32_t[]> data_len(new uint32_t[n]);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        hyobfs_udp_meta& m = meta[i];
        m.session_id = rd32();
        m.packet_id = (uint16_t)rd32();
        m.reserved_ = 0;
        m.max_size = rd32();
        m.addr_len = rd32();
        m.addr_off = rd64();
        data_len[i] = rd32();
        data_off[i] = total;
        total += data_len[i];
    }
    std::unique_ptr<uint8_t[]> data(new uint8_t[total ? total : 1]);
    need(data.get(), total);
    std::vector<uint8_t> sdata, saddrs;   // spread: slots with poisoned gaps
    auto slot = [](uint64_t len) { return (len + 8) / 8 * 8; };   // at least one poisoned byte after each
    if (spread) {
        uint64_t dt = 0, at = 0;
        for (uint32_t i = 0; i < n; ++i) {
            dt += slot(data_len[i]);
            at += slot(meta[i].addr_len);
        }
        sdata.assign(dt + 8, 0xEE);
        saddrs.assign(at + 8, 0xEE);
        dt = at = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (data_len[i]) memcpy(sdata.data() + dt, data.get() + data_off[i], data_len[i]);
            if (meta[i].addr_len) memcpy(saddrs.data() + at, addrs.get() + meta[i].addr_off, meta[i].addr_len);
            data_off[i] = dt;
            meta[i].addr_off = at;
            ASAN_POISON_MEMORY_REGION(sdata.data() + dt + data_len[i], slot(data_len[i]) - data_len[i]);
            ASAN_POISON_MEMORY_REGION(saddrs.data() + at + meta[i].addr_len, slot(meta[i].addr_len) - meta[i].addr_len);
            dt += slot(data_len[i]);
            at += slot(meta[i].addr_len);
        }
    }
    const uint8_t* const p_data = spread ? sdata.data() : data.get();
    const uint8_t* const p_addrs = spread ? saddrs.data() : addrs.get();
    auto status = filled<int32_t>(n);
    auto first = filled<uint64_t>((size_t)n + 1);
    auto totals = filled<uint64_t>(2);
    auto dgram_off = filled<uint64_t>(dgram_cap);
    auto dgram_len = filled<uint32_t>(dgram_cap);
    auto out = filled<uint8_t>(out_cap ? mis + out_cap : 0);
    const uint64_t ws_bytes = hyobfs_udp_frag_workspace_size(n);
    std::unique_ptr<uint64_t[]> ws(new uint64_t[ws_bytes / 8]);
    const int32_t rc = hyobfs_udp_frag_batch(p_data, data_off.get(), data_len.get(), meta.get(), p_addrs, n,
                                             out ? out.get() + mis : nullptr, out_cap, dgram_off.get(), dgram_len.get(),
                                             dgram_cap, first.get(), status.get(), totals.get(), ws.get(), nullptr);
    if (spread) {
        ASAN_UNPOISON_MEMORY_REGION(sdata.data(), sdata.size());
        ASAN_UNPOISON_MEMORY_REGION(saddrs.data(), saddrs.size());
    }
    wr(&rc, 4);
    wr(status.get(), 4 * (size_t)n);
    wr(first.get(), 8 * ((size_t)n + 1));
    wr(totals.get(), 16);
    wr(dgram_off.get(), 8 * dgram_cap);
    wr(dgram_len.get(), 4 * dgram_cap);
    if (out) wr(out.get(), mis + out_cap);
}

static void op_parse() {
    Datagrams d;
    d.read();
    const size_t n = d.len.size();
    auto out = filled<hyobfs_udp_parsed>(n);
    const int32_t rc = hyobfs_udp_parse_batch(d.buf.data(), d.off.data(), d.len.data(), n, out.get(), nullptr);
    wr(&rc, 4);
    wr(out.get(), n * sizeof(hyobfs_udp_parsed));
}

static void op_assemble() {
    Datagrams d;
    d.read();
    const size_t n = d.len.size();
    auto parsed = filled<hyobfs_udp_parsed>(n);
    const int32_t rc0 = hyobfs_udp_parse_batch(d.buf.data(), d.off.data(), d.len.data(), n, parsed.get(), nullptr);
    const uint32_t n_idx = rd32();
    std::unique_ptr<uint32_t[]> idx(new uint32_t[n_idx ? n_idx : 1]);
    need(idx.get(), 4 * (size_t)n_idx);
    const uint32_t m = rd32();
    std::unique_ptr<uint64_t[]> msg_first(new uint64_t[(size_t)m + 1]);
    need(msg_first.get(), 8 * ((size_t)m + 1));
    std::unique_ptr<uint64_t[]> out_off(new uint64_t[m]);
    std::unique_ptr<uint32_t[]> out_cap(new uint32_t[m]);
    uint64_t total = 0;
    for (uint32_t j = 0; j < m; ++j) {
        out_cap[j] = rd32();
        total += rd32();
        out_off[j] = total;
        total += out_cap[j];
    }
    auto out = filled<uint8_t>(total ? total : 1);
    auto out_len = filled<uint32_t>(m);
    auto status = filled<int32_t>(m);
    const int32_t rc = hyobfs_udp_assemble_batch(d.buf.data(), d.off.data(), parsed.get(), n, idx.get(), msg_first.get(), m,
                                                 out.get(), out_off.get(), out_cap.get(), out_len.get(), status.get(),
                                                 nullptr);
    wr(&rc0, 4);
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
            op_frag();
        else if (kind == 2)
            op_parse();
        else if (kind == 3)
            op_assemble();
        else
            return 2;
    }
    fclose(g_f);
    if (fclose(g_o) != 0) return 2;
    printf("done\n");
    return 0;
}
