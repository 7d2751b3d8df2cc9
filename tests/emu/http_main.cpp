// http_main.cpp -- stand-alone driver of the HTTP / TCP sniff entry points on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_http_sniff.py compiles this file together
// with hysteria_amd/csrc/sniff.hip and quic.hip for the host against hip_emu.h
// (-DHYOBFS_EMULATE) under AddressSanitizer and runs it as a child process.
//
//   http_main CASES
// CASES: u32 mode (0 http_request_host, 1 tcp_sniff, 2 tcp_sniff next to
// tls_record_sni), u32 n, u32 name_stride, then n x (u32 len, bytes), all
// little-endian.  Streams are laid out 8-byte aligned with the bytes between
// them poisoned, so a read past a stream's end stops the program; `names` is
// filled with 0xA5, `res` with 0xFF, and both are printed whole.  One line per
// stream:
//   status name_len name_off need <name row as hex>
// in mode 2 followed by the same five fields as hyobfs_tls_record_sni_batch
// leaves them on the same bytes; then `tail <byte after names> <bytes after res>`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs_sniff.h"

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t mode = rd32(f), n = rd32(f), stride = rd32(f);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n);
    std::vector<std::vector<uint8_t>> msgs(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = rd32(f);
        msgs[i].resize(len[i]);
        if (len[i] && fread(msgs[i].data(), 1, len[i], f) != len[i]) return 2;
        off[i] = total;
        total += ((uint64_t)len[i] + 1 + 7) / 8 * 8;   // at least one poisoned byte after each stream
    }
    fclose(f);
    std::vector<uint8_t> buf(total + 8, 0xEE);
    for (uint32_t i = 0; i < n; ++i)
        if (len[i]) memcpy(buf.data() + off[i], msgs[i].data(), len[i]);
    for (uint32_t i = 0; i < n; ++i)
        ASAN_POISON_MEMORY_REGION(buf.data() + off[i] + len[i], (i + 1 < n ? off[i + 1] : total) - (off[i] + len[i]));
    std::vector<uint8_t> names((uint64_t)n * stride + 1, 0xA5), names2 = names;
    std::vector<hyobfs_sniff_result> res(n + 1), res2(n + 1);
    memset(res.data(), 0xFF, (n + 1) * sizeof(hyobfs_sniff_result));
    memset(res2.data(), 0xFF, (n + 1) * sizeof(hyobfs_sniff_result));
    int rc = mode == 0 ? hyobfs_http_request_host_batch(buf.data(), off.data(), len.data(), n, names.data(), stride,
                                                        res.data(), nullptr)
                       : hyobfs_tcp_sniff_batch(buf.data(), off.data(), len.data(), n, names.data(), stride,
                                                res.data(), nullptr);
    if (rc == HYOBFS_OK && mode == 2)
        rc = hyobfs_tls_record_sni_batch(buf.data(), off.data(), len.data(), n, names2.data(), stride, res2.data(),
                                         nullptr);
    for (uint32_t i = 0; i < n; ++i)
        ASAN_UNPOISON_MEMORY_REGION(buf.data() + off[i] + len[i], (i + 1 < n ? off[i + 1] : total) - (off[i] + len[i]));
    if (rc != HYOBFS_OK) {
        fprintf(stderr, "call failed: %d\n", rc);
        return 3;
    }
    for (uint32_t i = 0; i < n; ++i) {
        printf("%d %u %u %u ", res[i].status, res[i].name_len, res[i].name_off, res[i].need);
        for (uint32_t k = 0; k < stride; ++k) printf("%02x", names[(uint64_t)i * stride + k]);
        if (!stride) printf("-");
        if (mode == 2) {
            printf(" %d %u %u %u ", res2[i].status, res2[i].name_len, res2[i].name_off, res2[i].need);
            for (uint32_t k = 0; k < stride; ++k) printf("%02x", names2[(uint64_t)i * stride + k]);
        }
        printf("\n");
    }
    printf("tail %02x %08x%08x%08x%08x\n", names[(uint64_t)n * stride], (uint32_t)res[n].status, res[n].name_len,
           res[n].name_off, res[n].need);
    return 0;
}
