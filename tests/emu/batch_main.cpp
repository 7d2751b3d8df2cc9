// batch_main.cpp -- stand-alone driver of the Salamander batch kernels on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_batch_limits.py compiles this file under
// AddressSanitizer, links it against tests/emu/libhyobfs_emu.so (the kernel
// sources built for the host against hip_emu.h) and runs it as a child process:
// a program with its own main, nothing is preloaded.
//
//   batch_main CASES
// CASES (tests/batch_limit_cases.py writes it) is a run of sections, all
// little-endian, each opening with a u32 tag:
//   1 batch:  u32 name_len; name; u32 obfuscate, psk_len; psk; u64 n; u32 flags (1: in_off,
//             2: in_len), in_align (the input base modulo 16: 0 or 8); u64 in_stride;
//             u32 len_uniform, pkt_cap; u64 out_cap, out_stride, in_size; the input;
//             [n x u64 in_off]; [n x u32 in_len]; n x u64 salts; u32 settings and per
//             setting u32 HYOBFS_KERNEL_* to set, i32 expected answer of
//             hyobfs_salamander_batch_kernel; i32 expected status of the batch call;
//             n x u64 expected out_off; n x u32 expected out_len; u64 expected
//             out_total, regions and per region u64 offset, length and the bytes.
//             Prints, per setting, `<name> <setting> kernel=<answer> status=<status>
//             bad=<mismatching bytes of out> first=<position> meta=<mismatches among
//             out_off, out_len and out_total>`.
//   2 packet: u32 psk_len; psk; u64 L; salt (8); payload (L); u64 wire_len; the expected
//             wire of hyobfs_salamander_obfuscate (wire_len 0: the call must return 0);
//             a wire datagram of L bytes whose plain text is the payload's first L - 8
//             bytes; u64 plain_len (0: hyobfs_salamander_deobfuscate must return 0).
//             Prints `packet L=<L> obf=<returned> bad=<n> deobf=<returned> bad=<n>`.
// Every array lies in an allocation of exactly the size the header promises: the input
// ends at its last byte, `out` is out_cap bytes filled with a sentinel, the workspace is
// hyobfs_batch_workspace_bytes, out_off / out_len have n entries.  AddressSanitizer
// stops the program at the first byte read or written outside them; every byte of `out`
// outside the expected regions must still hold the sentinel.  The first line printed is
// `limit=<HYOBFS_BATCH_MAX_DATAGRAM>`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs.h"

static FILE* g_f;
static const uint8_t kSentinel = 0xA5, kUnset = 0xEE;

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
// an allocation of exactly `bytes` bytes (16-byte aligned, as malloc's are)
struct Exact {
    uint8_t* p;
    explicit Exact(uint64_t bytes) : p(static_cast<uint8_t*>(malloc(bytes ? bytes : 1))) {
        if (!p) {
            fprintf(stderr, "allocation of %llu bytes failed\n", (unsigned long long)bytes);
            exit(2);
        }
        if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) exit(2);
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

static int run_batch() {
    const uint32_t name_len = rd32();
    std::string name(name_len, ' ');
    rd(&name[0], name_len);
    const uint32_t obf = rd32(), psk_len = rd32();
    std::vector<uint8_t> psk(psk_len);
    rd(psk.data(), psk_len);
    const uint64_t n = rd64();
    const uint32_t flags = rd32(), in_align = rd32();
    const uint64_t in_stride = rd64();
    const uint32_t len_uniform = rd32(), pkt_cap = rd32();
    const uint64_t out_cap = rd64(), out_stride = rd64(), in_size = rd64();
    // the input: in_size bytes ending at the allocation's end, in_align bytes (poisoned) in front
    Exact in_buf(in_size + in_align);
    uint8_t* in = in_buf.p + in_align;
    rd(in, in_size);
    if (in_align) ASAN_POISON_MEMORY_REGION(in_buf.p, in_align);
    Exact off_buf(n * 8), len_buf(n * 4), salt_buf(n * 8);
    if (flags & 1) rd(off_buf.p, n * 8);
    if (flags & 2) rd(len_buf.p, n * 4);
    rd(salt_buf.p, n * 8);
    const uint32_t nset = rd32();
    std::vector<std::pair<uint32_t, int32_t>> settings(nset);
    for (auto& s : settings) {
        s.first = rd32();
        s.second = (int32_t)rd32();
    }
    const int32_t exp_status = (int32_t)rd32();
    std::vector<uint64_t> exp_off(n);
    std::vector<uint32_t> exp_len(n);
    rd(exp_off.data(), n * 8);
    rd(exp_len.data(), n * 4);
    const uint64_t exp_total = rd64(), nreg = rd64();
    std::vector<std::pair<uint64_t, std::vector<uint8_t>>> regions(nreg);
    for (auto& r : regions) {
        r.first = rd64();
        r.second.resize(rd64());
        rd(r.second.data(), r.second.size());
        if (r.first + r.second.size() > out_cap) return 2;
    }

    hyobfs_salamander* ctx = nullptr;
    if (hyobfs_salamander_new(psk.data(), psk_len, 0, &ctx) != HYOBFS_OK) {
        fprintf(stderr, "salamander_new failed\n");
        return 3;
    }
    static const char* kSettingName[4] = {"auto", "wave", "tile", "flat"};
    for (const auto& s : settings) {
        if (s.first > 3 || hyobfs_salamander_set_kernel(ctx, (int)s.first) != HYOBFS_OK) return 3;
        Exact out(out_cap), got_off(n * 8), got_len(n * 4), total(8);
        memset(out.p, kSentinel, out_cap);
        memset(got_off.p, kUnset, n * 8);
        memset(got_len.p, kUnset, n * 4);
        memset(total.p, kUnset, 8);
        hyobfs_batch b;
        memset(&b, 0, sizeof b);
        b.n = n;
        b.in = in;
        b.in_off = (flags & 1) ? reinterpret_cast<const uint64_t*>(off_buf.p) : nullptr;
        b.in_stride = in_stride;
        b.in_len = (flags & 2) ? reinterpret_cast<const uint32_t*>(len_buf.p) : nullptr;
        b.len_uniform = len_uniform;
        b.pkt_cap = pkt_cap;
        b.salts = reinterpret_cast<const uint64_t*>(salt_buf.p);
        b.out = out.p;
        b.out_cap = out_cap;
        b.out_stride = out_stride;
        b.out_off = reinterpret_cast<uint64_t*>(got_off.p);
        b.out_len = reinterpret_cast<uint32_t*>(got_len.p);
        b.out_total = reinterpret_cast<uint64_t*>(total.p);
        const uint64_t ws_bytes = hyobfs_batch_workspace_bytes(&b);
        Exact ws(ws_bytes);   // exactly the bytes asked for: an overrun is a heap-buffer-overflow
        b.workspace = ws_bytes ? ws.p : nullptr;
        b.workspace_bytes = ws_bytes;
        const int kernel = hyobfs_salamander_batch_kernel(ctx, &b, (int)obf);
        const int st = obf ? hyobfs_salamander_obfuscate_batch(ctx, &b, nullptr)
                           : hyobfs_salamander_deobfuscate_batch(ctx, &b, nullptr);
        // the whole of out: the regions' bytes, the sentinel everywhere else
        uint64_t bad = 0, meta = 0;
        long long first = -1;
        for (const auto& r : regions) {
            for (uint64_t i = 0; i < r.second.size(); ++i)
                if (out.p[r.first + i] != r.second[i] && bad++ == 0) first = (long long)(r.first + i);
            memset(out.p + r.first, kSentinel, r.second.size());   // regions do not overlap
        }
        for (uint64_t i = 0; i < out_cap; ++i)
            if (out.p[i] != kSentinel && bad++ == 0) first = (long long)i;
        for (uint64_t i = 0; i < n; ++i) {
            meta += reinterpret_cast<uint64_t*>(got_off.p)[i] != exp_off[i];
            meta += reinterpret_cast<uint32_t*>(got_len.p)[i] != exp_len[i];
        }
        meta += *reinterpret_cast<uint64_t*>(total.p) != exp_total;
        printf("%s %s kernel=%d status=%d bad=%llu first=%lld meta=%llu\n", name.c_str(), kSettingName[s.first], kernel,
               st, (unsigned long long)bad, first, (unsigned long long)meta);
        if (kernel != s.second || st != exp_status) fprintf(stderr, "%s: expected kernel %d status %d\n", name.c_str(), s.second, exp_status);
        fflush(stdout);
    }
    hyobfs_salamander_free(ctx);
    return 0;
}

static int run_packet() {
    const uint32_t psk_len = rd32();
    std::vector<uint8_t> psk(psk_len);
    rd(psk.data(), psk_len);
    const uint64_t L = rd64();
    uint8_t salt[8];
    rd(salt, 8);
    Exact payload(L);
    rd(payload.p, L);
    const uint64_t wire_len = rd64();
    Exact exp_wire(wire_len);
    rd(exp_wire.p, wire_len);
    Exact wire_in(L);
    rd(wire_in.p, L);
    const uint64_t plain_len = rd64();
    hyobfs_salamander* ctx = nullptr;
    if (hyobfs_salamander_new(psk.data(), psk_len, 0, &ctx) != HYOBFS_OK) return 3;
    uint64_t bad1 = 0, bad2 = 0;
    Exact out(L + 8);
    memset(out.p, kSentinel, L + 8);
    const size_t w = hyobfs_salamander_obfuscate(ctx, payload.p, L, salt, out.p, L + 8);
    if (w == wire_len) {
        for (uint64_t i = 0; i < wire_len; ++i) bad1 += out.p[i] != exp_wire.p[i];
        for (uint64_t i = wire_len; i < L + 8; ++i) bad1 += out.p[i] != kSentinel;
    } else {
        bad1 = 1;
    }
    Exact back(L);
    memset(back.p, kSentinel, L);
    const size_t d = hyobfs_salamander_deobfuscate(ctx, wire_in.p, L, back.p, L);
    if (d == plain_len) {
        for (uint64_t i = 0; i < plain_len; ++i) bad2 += back.p[i] != payload.p[i];
        for (uint64_t i = plain_len; i < L; ++i) bad2 += back.p[i] != kSentinel;
    } else {
        bad2 = 1;
    }
    hyobfs_salamander_free(ctx);
    printf("packet L=%llu obf=%zu bad=%llu deobf=%zu bad=%llu\n", (unsigned long long)L, w, (unsigned long long)bad1, d,
           (unsigned long long)bad2);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    g_f = fopen(argv[1], "rb");
    if (!g_f) return 2;
    printf("limit=%u\n", (unsigned)HYOBFS_BATCH_MAX_DATAGRAM);
    uint32_t tag;
    while (fread(&tag, 1, 4, g_f) == 4) {
        const int rc = tag == 1 ? run_batch() : tag == 2 ? run_packet() : 2;
        if (rc) return rc;
    }
    fclose(g_f);
    printf("done\n");
    return 0;
}
