// acl_index_main.cpp -- stand-alone driver of the ACL entry points on the CPU for
// rule sets with indexed DOMAIN_SETs: acl_regex_main.cpp over
// hyobfs_acl_ruleset_new_opts.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_acl_index.py compiles this file together
// with hysteria_amd/csrc/acl.hip for the host against hip_emu.h
// (-DHYOBFS_EMULATE) under AddressSanitizer, once as it is and once with
// -DHY_ACL_INDEX_HASH_BITS=2, and runs it as a child process.
//
//   acl_index_main CASES FLAGS INDEX_MIN [STRUCT_SIZE RESERVED]
// FLAGS, INDEX_MIN: hyobfs_acl_options.flags and .index_min, in decimal; FLAGS
// "null": opts == NULL.  STRUCT_SIZE, RESERVED: those fields, if not
// sizeof(hyobfs_acl_options) and 0.
// CASES (tests/acl_cases.py writes it), all little-endian: u32 n_groups, then per
// group
//   u32 mode (0 match_batch, 1 match_sniffed_batch), n_rules, n_items,
//       name_stride (mode 1), null_ips (1: the three address pointers are null)
//   n_rules x rule:  u32 kind, proto, start_port, end_port, outbound, hijack,
//       pattern_len (0xFFFFFFFF: a null pattern), pattern bytes, 16 address
//       bytes, u8 family, prefix, inverse, 0, u32 n_entries, entries_null, then
//       per entry (DOMAIN_SET) u32 type, len, bytes or (CIDR_SET) 16 address
//       bytes, u8 family, prefix, 0, 0
//   n_items x item:  u32 name_len, bytes, 4 ipv4 bytes, 16 ipv6 bytes, u8 flags,
//       proto, u16 port, i32 sniff status (mode 1)
// Names are laid out with the bytes between them poisoned (mode 0: 8-byte
// aligned slots; mode 1: rows of name_stride bytes, everything past a name, and
// the whole row of an item without a name, poisoned), so a read past a name
// stops the program.  `res` holds exactly n_items records, pre-filled with
// 0xFF.  Output: per group `group <rc of ruleset_new_opts> <bad rule> <bad entry>
// <rule count> <entries of the walk table>`, then, when the set was made, one
// line `index <rule> <values> <slots> <max_probe>` per rule that has an index,
// then one line per item: status rule outbound hijack.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/hyobfs_acl.h"

static FILE* g_f;

static void rd(void* p, size_t n) {
    if (n && fread(p, 1, n, g_f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
}
static uint32_t rd32() {
    uint8_t b[4];
    rd(b, 4);
    return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
}
static uint8_t rd8() {
    uint8_t b;
    rd(&b, 1);
    return b;
}

int main(int argc, char** argv) {
    if (argc != 4 && argc != 6) return 2;
    const bool null_opts = strcmp(argv[2], "null") == 0;
    hyobfs_acl_options opts{(uint32_t)sizeof(hyobfs_acl_options), (uint32_t)strtoul(argv[2], nullptr, 10),
                            (uint32_t)strtoul(argv[3], nullptr, 10), 0};
    if (argc == 6) {
        opts.struct_size = (uint32_t)strtoul(argv[4], nullptr, 10);
        opts.reserved = (uint32_t)strtoul(argv[5], nullptr, 10);
    }
    g_f = fopen(argv[1], "rb");
    if (!g_f) return 2;
    const uint32_t n_groups = rd32();
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t mode = rd32(), n_rules = rd32(), n = rd32(), stride = rd32(), null_ips = rd32();
        std::vector<hyobfs_acl_rule> rules(n_rules);
        // every pattern, value and entry list in an allocation of exactly its size
        std::vector<std::unique_ptr<uint8_t[]>> bytes;
        std::vector<std::unique_ptr<hyobfs_acl_domain[]>> dlists;
        std::vector<std::unique_ptr<hyobfs_acl_cidr[]>> clists;
        auto blob = [&](uint32_t len) {
            bytes.emplace_back(new uint8_t[len ? len : 1]);
            rd(bytes.back().get(), len);
            return bytes.back().get();
        };
        for (auto& r : rules) {
            memset(&r, 0, sizeof r);
            r.kind = rd32();
            r.proto = rd32();
            r.start_port = (uint16_t)rd32();
            r.end_port = (uint16_t)rd32();
            r.outbound = rd32();
            r.hijack = rd32();
            r.pattern_len = rd32();
            if (r.pattern_len == 0xFFFFFFFFu) {
                r.pattern_len = 0;
                r.pattern = nullptr;
            } else {
                r.pattern = blob(r.pattern_len);
            }
            rd(r.addr, 16);
            r.family = rd8();
            r.prefix = rd8();
            r.inverse = rd8();
            rd8();
            r.n_entries = rd32();
            const uint32_t entries_null = rd32();
            if (r.kind == HYOBFS_ACL_DOMAIN_SET) {
                dlists.emplace_back(new hyobfs_acl_domain[r.n_entries ? r.n_entries : 1]);
                for (uint32_t k = 0; k < r.n_entries; ++k) {
                    auto& d = dlists.back()[k];
                    d.type = rd32();
                    d.len = rd32();
                    d.value = blob(d.len);
                }
                r.entries = entries_null ? nullptr : dlists.back().get();
            } else if (r.kind == HYOBFS_ACL_CIDR_SET) {
                clists.emplace_back(new hyobfs_acl_cidr[r.n_entries ? r.n_entries : 1]);
                for (uint32_t k = 0; k < r.n_entries; ++k) {
                    auto& c = clists.back()[k];
                    rd(c.addr, 16);
                    c.family = rd8();
                    c.prefix = rd8();
                    c.pad_[0] = rd8();
                    c.pad_[1] = rd8();
                }
                r.entries = entries_null ? nullptr : clists.back().get();
            }
        }
        std::vector<std::vector<uint8_t>> names(n);
        std::vector<uint64_t> off(n);
        std::vector<uint32_t> len(n);
        std::vector<uint8_t> v4(4 * (size_t)n), v6(16 * (size_t)n), flags(n), proto(n);   // exact: ASan sees an overrun
        std::vector<uint16_t> port(n);
        std::vector<hyobfs_sniff_result> sres(n);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; ++i) {
            len[i] = rd32();
            names[i].resize(len[i]);
            rd(names[i].data(), len[i]);
            rd(&v4[4 * (size_t)i], 4);
            rd(&v6[16 * (size_t)i], 16);
            flags[i] = rd8();
            proto[i] = rd8();
            uint8_t p[2];
            rd(p, 2);
            port[i] = (uint16_t)(p[0] | p[1] << 8);
            sres[i] = hyobfs_sniff_result{(int32_t)rd32(), len[i], 7, 0};
            off[i] = mode == 0 ? total : (uint64_t)i * stride;
            total += mode == 0 ? (len[i] + 1 + 7) / 8 * 8 : stride;
        }
        hyobfs_acl_ruleset* set = nullptr;
        const int rc = hyobfs_acl_ruleset_new_opts(n_rules ? rules.data() : nullptr, n_rules, 0,
                                                   null_opts ? nullptr : &opts, &set);
        printf("group %d %lld %lld %u %u\n", rc, (long long)hyobfs_acl_ruleset_bad_rule(),
               (long long)hyobfs_acl_ruleset_bad_entry(), hyobfs_acl_ruleset_rules(set), hyobfs_acl_ruleset_entries(set));
        if (rc != HYOBFS_OK) continue;
        for (uint32_t r = 0; r < n_rules; ++r) {
            hyobfs_acl_index_info info;
            if (hyobfs_acl_ruleset_index_info(set, r, &info) != HYOBFS_OK) return 3;
            if (info.slots) printf("index %u %u %u %u\n", r, info.values, info.slots, info.max_probe);
        }
        hyobfs_acl_index_info none;
        if (hyobfs_acl_ruleset_index_info(set, n_rules, &none) != HYOBFS_ERR_INVALID) return 3;
        // the rules may be freed after the call
        bytes.clear();
        dlists.clear();
        clists.clear();
        rules.clear();
        rules.shrink_to_fit();
        std::vector<uint8_t> buf(total + 8, 0xEE);
        for (uint32_t i = 0; i < n; ++i) {
            // a sniffed name longer than its row was never written (NAME_CAP)
            const bool have = mode == 0 || (sres[i].status == HYOBFS_OK && len[i] <= stride);
            const uint64_t used = have ? len[i] : 0, slot = mode == 0 ? (len[i] + 1 + 7) / 8 * 8 : stride;
            if (used) memcpy(buf.data() + off[i], names[i].data(), used);
            ASAN_POISON_MEMORY_REGION(buf.data() + off[i] + used, slot - used);
        }
        std::vector<hyobfs_acl_result> res(n);
        memset(res.data(), 0xFF, n * sizeof(hyobfs_acl_result));
        const uint8_t *p4 = null_ips ? nullptr : v4.data(), *p6 = null_ips ? nullptr : v6.data(),
                      *pf = null_ips ? nullptr : flags.data();
        int st;
        if (mode == 0)
            st = hyobfs_acl_match_batch(set, buf.data(), off.data(), len.data(), p4, p6, pf, proto.data(), port.data(), n,
                                        res.data(), nullptr);
        else
            st = hyobfs_acl_match_sniffed_batch(set, buf.data(), stride, sres.data(), p4, p6, pf, proto.data(),
                                                port.data(), n, res.data(), nullptr);
        ASAN_UNPOISON_MEMORY_REGION(buf.data(), buf.size());
        hyobfs_acl_ruleset_free(set);
        if (st != HYOBFS_OK) {
            fprintf(stderr, "call failed: %d\n", st);
            return 3;
        }
        for (uint32_t i = 0; i < n; ++i)
            printf("%d %d %u %u\n", res[i].status, res[i].rule, res[i].outbound, res[i].hijack);
    }
    fclose(g_f);
    printf("done\n");
    return 0;
}
