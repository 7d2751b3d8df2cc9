// plan_main.cpp -- the host-side launch plan of the Salamander batch calls as a table.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_batch_plan.py compiles this file under
// AddressSanitizer, links it against tests/emu/libhyobfs_emu.so and runs it as a child
// process with nothing preloaded, once per environment (the kernel knobs are read once
// per process).  It launches nothing: it walks a fixed lattice of batch descriptions and
// prints, per description, one row
//   <hyobfs_batch_workspace_bytes> then, for the context settings 0..3
//   (hyobfs_salamander_set_kernel), hyobfs_salamander_batch_kernel for obfuscate and
//   for deobfuscate
// The calls dereference no batch pointer; the pointers still come from small real
// allocations, 16-byte aligned, plus 8 for the misaligned cases.
//
// The lattice, outermost axis first (tests/test_batch_plan.py restates the sizes):
//   out        16-byte aligned, 8 past it (refused)
//   out_stride 0, 1201, 1208, 4096, HYOBFS_BATCH_MAX_DATAGRAM, that + 1
//   salts      present, absent
//   n          0, 1, 2, 255, 256, 257, 65537
//   input      explicit in_off (with in_len); in_stride 1200 with len_uniform; in_stride
//              1200 with in_len; contiguous (in_stride 0 with in_len); in_stride 0 without
//              in_len
//   workspace  absent, exactly hyobfs_batch_workspace_bytes, one byte short
//   in         16-byte aligned, 8 past it
//   out_cap    full (n slots, or n x 1209 packed), half of it
//   pkt_cap    0, 64
//   len_uniform 1200, 1201
// (the order that leaves the longest runs of equal rows: the recorded table is run-length
// coded, tests/golden/batch_plan.json)
// The first line printed is `rows=<count>`, the last `done`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../include/hyobfs.h"

int main() {
    static const uint8_t psk[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    hyobfs_salamander* ctx = nullptr;
    if (hyobfs_salamander_new(psk, sizeof psk, 0, &ctx) != HYOBFS_OK) return 3;
    uint8_t* in = static_cast<uint8_t*>(aligned_alloc(16, 64));
    uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, 64));
    uint8_t* ws = static_cast<uint8_t*>(aligned_alloc(16, 64));
    uint64_t* in_off = static_cast<uint64_t*>(aligned_alloc(16, 64));
    uint32_t* in_len = static_cast<uint32_t*>(aligned_alloc(16, 64));
    uint64_t* salts = static_cast<uint64_t*>(aligned_alloc(16, 64));
    if (!in || !out || !ws || !in_off || !in_len || !salts) return 3;

    const uint64_t ns[] = {0, 1, 2, 255, 256, 257, 65537};
    const uint64_t strides[] = {0, 1201, 1208, 4096, HYOBFS_BATCH_MAX_DATAGRAM, (uint64_t)HYOBFS_BATCH_MAX_DATAGRAM + 1};
    printf("rows=%d\n", 2 * 2 * 3 * 7 * 5 * 6 * 2 * 2 * 2 * 2);
    for (int out_mis = 0; out_mis < 2; ++out_mis)
    for (uint64_t stride : strides)
    for (int no_salts = 0; no_salts < 2; ++no_salts)
    for (uint64_t n : ns)
    for (int layout = 0; layout < 5; ++layout)
    for (int wsmode = 0; wsmode < 3; ++wsmode)
    for (int in_mis = 0; in_mis < 2; ++in_mis)
    for (int half = 0; half < 2; ++half)
    for (uint32_t pkt_cap : {0u, 64u})
    for (uint32_t len : {1200u, 1201u}) {
        hyobfs_batch b{};
        b.n = n;
        b.in = in + 8 * in_mis;
        b.in_off = layout == 0 ? in_off : nullptr;
        b.in_stride = layout == 1 || layout == 2 ? 1200 : 0;
        b.in_len = layout == 0 || layout == 2 || layout == 3 ? in_len : nullptr;
        b.len_uniform = len;
        b.pkt_cap = pkt_cap;
        b.salts = no_salts ? nullptr : salts;
        b.out = out + 8 * out_mis;
        b.out_cap = (n * (stride ? stride : 1209)) >> half;
        b.out_stride = stride;
        const uint64_t need = hyobfs_batch_workspace_bytes(&b);
        b.workspace = wsmode ? ws : nullptr;
        b.workspace_bytes = wsmode == 2 && need ? need - 1 : wsmode ? need : 0;
        printf("%llu", (unsigned long long)need);
        for (int k = 0; k < 4; ++k) {
            if (hyobfs_salamander_set_kernel(ctx, k) != HYOBFS_OK) return 3;
            printf(" %d %d", hyobfs_salamander_batch_kernel(ctx, &b, 1), hyobfs_salamander_batch_kernel(ctx, &b, 0));
        }
        printf("\n");
    }
    puts("done");
    free(salts);
    free(in_len);
    free(in_off);
    free(ws);
    free(out);
    free(in);
    hyobfs_salamander_free(ctx);
    return 0;
}
