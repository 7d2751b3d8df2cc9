// sniff_main.cpp -- stand-alone driver of the SNI entry points on the CPU.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_sniff.py compiles this file together
// with hysteria_amd/csrc/sniff.hip and quic.hip for the host against hip_emu.h
// (-DHYOBFS_EMULATE) under AddressSanitizer and runs it as a child process.
//
//   sniff_main CASES
// CASES: u32 mode (0 hello, 1 tls record, 2 quic), u32 n, u32 name_stride,
// u32 crypto_cap, then n x (u32 len, bytes), all little-endian.  Messages are
// laid out 8-byte aligned with the bytes between them poisoned, so a read past
// a message's end stops the program; `names` is filled with 0xA5 and printed
// whole.  One line per message:
//   status name_len name_off need <name row as hex>
// and in mode 2 also: qstatus out_len, then a last line `same 1` when qres,
// crypto and the packets equal what hyobfs_quic_read_crypto_payload_batch
// alone leaves on a copy of the input.
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
    const uint32_t mode = rd32(f), n = rd32(f), stride = rd32(f), cap = rd32(f);
    std::vector<std::vector<uint8_t>> msgs(n);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = rd32(f);
        msgs[i].resize(len[i]);
        if (len[i] && fread(msgs[i].data(), 1, len[i], f) != len[i]) return 2;
        off[i] = total;
        total += (len[i] + 1 + 7) / 8 * 8;   // at least one poisoned byte after each message
    }
    fclose(f);
    std::vector<uint8_t> buf(total + 8, 0xEE);
    for (uint32_t i = 0; i < n; ++i)
        if (len[i]) memcpy(buf.data() + off[i], msgs[i].data(), len[i]);
    std::vector<uint8_t> copy = buf;
    auto poison = [&](std::vector<uint8_t>& b, bool on) {
        for (uint32_t i = 0; i < n; ++i) {
            uint8_t* gap = b.data() + off[i] + len[i];
            const uint64_t end = i + 1 < n ? off[i + 1] : total;
            if (on) ASAN_POISON_MEMORY_REGION(gap, end - (off[i] + len[i]));
            else ASAN_UNPOISON_MEMORY_REGION(gap, end - (off[i] + len[i]));
        }
    };
    std::vector<uint8_t> names((uint64_t)n * stride + 1, 0xA5);
    std::vector<hyobfs_sniff_result> res(n);
    memset(res.data(), 0xFF, n * sizeof(hyobfs_sniff_result));
    std::vector<hyobfs_quic_result> qres(n), qres2(n);
    std::vector<uint8_t> crypto, crypto2;
    std::vector<uint64_t> coff(n);
    std::vector<uint32_t> ccap(n, cap);
    int rc, same = 1;
    poison(buf, true);
    if (mode == 0) {
        rc = hyobfs_tls_client_hello_sni_batch(buf.data(), off.data(), len.data(), n, names.data(), stride, res.data(),
                                               nullptr);
    } else if (mode == 1) {
        rc = hyobfs_tls_record_sni_batch(buf.data(), off.data(), len.data(), n, names.data(), stride, res.data(),
                                         nullptr);
    } else {
        for (uint32_t i = 0; i < n; ++i) coff[i] = (uint64_t)i * cap;
        crypto.assign((uint64_t)n * cap + 1, 0xA5);
        crypto2 = crypto;
        std::vector<uint8_t> ws(hyobfs_quic_sniff_workspace_size(n) + 1), ws2(hyobfs_quic_workspace_size(n) + 1);
        rc = hyobfs_quic_sniff_batch(buf.data(), off.data(), len.data(), n, crypto.data(), coff.data(), ccap.data(),
                                     qres.data(), names.data(), stride, res.data(), ws.data(), nullptr);
        poison(copy, true);
        const int rc2 = hyobfs_quic_read_crypto_payload_batch(copy.data(), off.data(), len.data(), n, crypto2.data(),
                                                              coff.data(), ccap.data(), qres2.data(), ws2.data(),
                                                              nullptr);
        poison(copy, false);
        poison(buf, false);
        same = rc2 == rc && crypto == crypto2 && copy == buf &&
               memcmp(qres.data(), qres2.data(), n * sizeof(hyobfs_quic_result)) == 0;
    }
    if (rc != HYOBFS_OK) {
        fprintf(stderr, "call failed: %d\n", rc);
        return 3;
    }
    for (uint32_t i = 0; i < n; ++i) {
        printf("%d %u %u %u ", res[i].status, res[i].name_len, res[i].name_off, res[i].need);
        for (uint32_t k = 0; k < stride; ++k) printf("%02x", names[(uint64_t)i * stride + k]);
        if (mode == 2) printf(" %d %u", qres[i].status, qres[i].out_len);
        printf("\n");
    }
    if (mode == 2) printf("same %d\n", same);
    printf("tail %02x\n", names[(uint64_t)n * stride]);
    return 0;
}
