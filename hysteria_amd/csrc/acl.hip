// acl.hip -- the outbound ACL's rule matching over a batch of host names and
// addresses (include/hyobfs_acl.h, which states the match rules).
//
// Reference: apernet/hysteria extras/outbounds/acl: compiledRuleSetImpl.Match
// (compile.go:88-109), compiledRule.Match (:62-70), the host matchers of
// matchers.go:20-79 and matchers_v2geo.go:24-60, :121-161.
//
//   acl_kernel   one WAVE per item, four items per 256-thread workgroup, grid-
//                stride over groups of four, no barrier between the waves (the
//                shape of sniff.hip's sni_kernel).  The wave loads its name a
//                byte per lane, lower-cases it and stages it in LDS once, finds
//                the length without trailing dots and the names it leaves to
//                the host with ballots, then walks the rule set's flattened
//                entry table 64 entries per step: lane l tests entry base + l
//                (protocol, port, then the entry's matcher against the name in
//                LDS or the item's addresses in registers).  Entries are in
//                rule order, so the lowest set bit of the first non-zero ballot
//                is the first matching rule, and the wave stops there.
//
// The entry table: a rule of any kind but the two sets is one 32-byte entry; a
// DOMAIN_SET is one entry per value (FULL as an exact entry, ROOT as a suffix
// entry, PLAIN as a substring entry); a CIDR_SET is one entry whose lane runs
// the reference's binary search.  A REGEX value of a DOMAIN_SET is one entry too:
// its lane walks the value's DFA (acl_regex.h) over the name in LDS, and a rule's
// regex entries stand together after its other entries, so that their walks run
// side by side in as few steps as possible.  A domain entry carries the end of its
// pattern (16 bytes) next to its lengths, and the wave keeps the end of its name in
// registers, so all but a near miss is decided without touching the pattern
// bytes in memory.  Addresses are kept as four big-endian words
// in v4-mapped form, so Equal and Contains with their To4 rules become word
// compares (hyobfs_acl.h, traps 1 to 3).
//
// The index (hyobfs_acl_ruleset_new_opts with HYOBFS_ACL_FLAG_INDEX): the FULL and ROOT
// values of a large enough DOMAIN_SET are not entries of the walk but one entry of kind
// kDomainIndex in front of the set's PLAIN and REGEX entries.  Its lane hashes the name
// in LDS from its end towards its start, and at position 0 and after every '.' looks the
// suffix that begins there up in the set's open-addressed table of 16-byte slots (hash,
// offset of the value's bytes, length and type bits): the candidates of hyobfs_acl.h,
// "THE INDEX".  A hash hit is never a match by itself: the value's bytes are compared.
#include <algorithm>
#include <string>
#include <utility>
#include <new>
#include <vector>

#include "kernels.h"
#include "acl_regex.h"
#include "../../include/hyobfs_acl.h"

namespace hyobfs {
namespace acl {

constexpr uint32_t kWaves = 4;   // items per workgroup
// Workgroups per launch, as sni_kernel's: far more than are resident at once (8 per CU
// at 8 waves per SIMD, 2048 on the chip), so that the dispatcher evens out items whose
// walks differ in length by orders of magnitude.
#ifndef HY_ACL_GRID_CAP
#define HY_ACL_GRID_CAP (1u << 16)
#endif
constexpr uint32_t kGridCap = HY_ACL_GRID_CAP;
constexpr uint32_t kNameLds = 256;   // HYOBFS_ACL_MAX_NAME rounded up to whole rounds of 64 lanes

// Test knob: only the low HY_ACL_INDEX_HASH_BITS bits of an index hash survive, in the stored
// hash and in the slot choice alike.  The emulated tier builds a second binary with 2, in which
// every chain is long and wraps round the table's end.
#ifndef HY_ACL_INDEX_HASH_BITS
#define HY_ACL_INDEX_HASH_BITS 32
#endif
static_assert(HY_ACL_INDEX_HASH_BITS >= 1 && HY_ACL_INDEX_HASH_BITS <= 32, "HY_ACL_INDEX_HASH_BITS");
constexpr uint32_t kIxHashMask = HY_ACL_INDEX_HASH_BITS >= 32 ? 0xFFFFFFFFu : (1u << (HY_ACL_INDEX_HASH_BITS & 31)) - 1;

enum : uint32_t { kAll = 0, kIp, kCidr4, kCidr6, kExact, kWildcard, kSuffix, kPlain, kCidrSet, kRegex, kDomainIndex };
enum { kBatch = 0, kSniffed = 1 };

struct alignas(16) Entry {
    uint32_t rule;
    uint32_t off;    // pattern: byte offset in `pats`; address / CIDR set: word offset in `words`;
                     // kRegex: cell offset in `dfa`
    uint16_t len;    // pattern length; kCidr4 / kCidr6: leading bits of the 128 that must agree
    uint8_t kind, proto;
    uint16_t start_port, end_port;
    // A piece of the pattern inside the entry, so that nearly every entry is decided without
    // a dependent load from `pats`.  Byte k of the 16 is bits 8 * (k % 4) of word k / 4.
    //   kExact / kSuffix  the last min(len, 16) pattern bytes, the last one first
    //   kWildcard         words 0-2: the literal bytes after the last '*', the last min(.., 12)
    //                     of them, the last one first; word 3: the shortest name the pattern
    //                     takes (len less its stars) | that count of literal bytes << 16
    //   kPlain            word 0: the first min(len, 4) bytes of the value, in order
    //   kRegex            word 0: the start state (0, rx::kAccept or rx::kDead)
    //   kDomainIndex      word 0: the table's slot count - 1 (`off`: its first slot in `slots`)
    uint32_t tail[4];
};
static_assert(sizeof(Entry) == 32, "Entry layout");
constexpr uint32_t kTail = 16, kWildTail = 12, kPlainHead = 4;

// One slot of an indexed set's table: one aligned 16-byte load.  A slot in use holds one distinct
// value; `meta` 0 is an empty slot and ends a probe sequence.
struct alignas(16) Slot {
    uint32_t hash;   // ix_hash of the value: a slot with another hash is passed without a dependent load
    uint32_t off;    // the value's bytes in `pats`
    uint32_t meta;   // the value's length | kIxFull and / or kIxRoot | kIxUsed
    uint32_t pad_;
};
static_assert(sizeof(Slot) == 16, "Slot layout");
constexpr uint32_t kIxLen = 0xFFFF, kIxFull = 1u << 16, kIxRoot = 1u << 17, kIxUsed = 1u << 31;

struct RuleOut {
    uint32_t outbound, hijack;
};

struct Args {
    const Entry* entries;
    const RuleOut* rule_out;
    const uint32_t* words;
    const uint8_t* pats;
    const uint16_t* dfa;
    const Slot* slots;
    uint32_t n_entries;
    const uint8_t* names;
    const uint64_t* name_off;          // kBatch
    const uint32_t* name_len;          // kBatch
    uint32_t name_stride;              // kSniffed
    const hyobfs_sniff_result* sres;   // kSniffed
    const uint8_t *ipv4, *ipv6, *ip_flags, *proto;
    const uint16_t* port;
    uint64_t n;
    hyobfs_acl_result* res;
};

// An item's addresses as net.IP.To16 would give them, in big-endian words.
struct Host {
    uint32_t a[4], b[4];   // IPv4 (v4-mapped), IPv6
    bool has_a, has_b;
    bool b4;               // IPv6 is v4-mapped: To4 reduces it to 4 bytes
};

HY_HD uint32_t be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// the first `bits` (0..128) of x and y agree
HY_HD bool prefix_eq(const uint32_t* x, const uint32_t* y, uint32_t bits) {
    bool eq = true;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t nb = bits > 32 * w ? (bits - 32 * w < 32 ? bits - 32 * w : 32) : 0;
        const uint32_t mask = nb ? 0xFFFFFFFFu << (32 - nb) : 0;
        eq &= ((x[w] ^ y[w]) & mask) == 0;
    }
    return eq;
}

// x < y as bytes.Compare of the 16 bytes
HY_HD bool words_less(const uint32_t* x, const uint32_t* y) {
    for (uint32_t w = 0; w < 4; ++w)
        if (x[w] != y[w]) return x[w] < y[w];
    return false;
}

// geoipMatcher.matchIP (matchers_v2geo.go:24-46) over one CIDR set: s[0] family-4
// entries {address, prefix} from s[4], then s[1] family-6 entries {address words,
// prefix | never << 8}.  `never`: the entry's address is v4-mapped, so Contains reduces
// it to 4 bytes and a 16-byte IP is never inside it.
HY_HD bool cidr_set_has(const uint32_t* s, const uint32_t* ip, bool is4) {
    int32_t left = 0;
    if (is4) {
        const uint32_t* t = s + 4;
        const uint32_t v = ip[3];
        int32_t right = (int32_t)s[0] - 1;
        while (left <= right) {
            const int32_t mid = (left + right) / 2;
            const uint32_t e = t[2 * mid], p = t[2 * mid + 1];
            const uint32_t mask = p ? 0xFFFFFFFFu << (32 - p) : 0;
            if (((e ^ v) & mask) == 0) return true;
            if (e < v) left = mid + 1;
            else right = mid - 1;
        }
        return false;
    }
    const uint32_t* t = s + 4 + 2 * (uint64_t)s[0];
    int32_t right = (int32_t)s[1] - 1;
    while (left <= right) {
        const int32_t mid = (left + right) / 2;
        const uint32_t* q = t + 5 * (uint64_t)mid;
        const uint32_t e[4] = {q[0], q[1], q[2], q[3]};
        if (!(q[4] >> 8) && prefix_eq(e, ip, q[4] & 0xFF)) return true;
        if (words_less(e, ip)) left = mid + 1;
        else right = mid - 1;
    }
    return false;
}

// the first `n` (0..16) bytes of the two 16-byte pieces agree
HY_HD bool tail_eq(const uint32_t* x, const uint32_t* y, uint32_t n) {
    bool eq = true;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t nb = n > 4 * w ? (n - 4 * w < 4 ? n - 4 * w : 4) : 0;
        const uint32_t mask = nb == 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1;
        eq &= ((x[w] ^ y[w]) & mask) == 0;
    }
    return eq;
}

// name[at, at + pl) == p[0, pl), compared from the end (names differ there first)
HY_HD bool bytes_eq(const uint8_t* name, uint32_t at, const uint8_t* p, uint32_t pl) {
    for (uint32_t k = pl; k-- > 0;)
        if (name[at + k] != p[k]) return false;
    return true;
}

// deepMatchRune (matchers.go:58-73) in the iterative form: on a mismatch go back to
// the last '*' and let it take one more byte.  O(nl * pl).
HY_HD bool wildcard(const uint8_t* name, uint32_t nl, const uint8_t* p, uint32_t pl) {
    uint32_t s = 0, q = 0, star = 0xFFFFFFFFu, mark = 0;
    while (s < nl) {
        const uint32_t pc = q < pl ? p[q] : 0x100;
        if (pc == '*') {
            star = q++;
            mark = s;
        } else if (pc == name[s]) {
            ++s;
            ++q;
        } else if (star != 0xFFFFFFFFu) {
            q = star + 1;
            s = ++mark;
        } else {
            return false;
        }
    }
    while (q < pl && p[q] == '*') ++q;
    return q == pl;
}

// ---- the index of a DOMAIN_SET's FULL and ROOT values
// The hash runs from a text's last byte to its first (FNV-1a's step), so one backward pass over
// a name gives the hash of every suffix; ix_mix spreads it before a slot is taken from its low
// bits.
constexpr uint32_t kIxBasis = 2166136261u;
HY_HD uint32_t ix_step(uint32_t h, uint32_t c) { return (h ^ c) * 16777619u; }
HY_HD uint32_t ix_mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h & kIxHashMask;
}
HY_HD uint32_t ix_hash(const uint8_t* v, uint32_t len) {
    uint32_t h = kIxBasis;
    for (uint32_t k = len; k-- > 0;) h = ix_step(h, v[k]);
    return ix_mix(h);
}

// The candidate name[at, nl) with hash `hash` against one table of mask + 1 slots: linear probing
// from slot hash & mask DOWNWARDS (so that the weak-hash build, whose sequences all begin in the
// first slots, goes round the table's end at once) to the first empty slot; the table is at most
// half full, so there is one.  Values are distinct: the slot whose bytes agree decides, by its
// type bits (FULL only for the whole name).
HY_HD bool index_probe(const Slot* slots, uint32_t mask, const uint8_t* pats, const uint8_t* name, uint32_t at,
                       uint32_t nl, uint32_t hash) {
    const uint32_t len = nl - at, want = at == 0 ? kIxFull | kIxRoot : kIxRoot;
    for (uint32_t s = hash & mask;; s = (s - 1) & mask) {
        const Slot x = slots[s];
        if (!x.meta) return false;
        if (x.hash == hash && (x.meta & kIxLen) == len && bytes_eq(name, at, pats + x.off, len)) return (x.meta & want) != 0;
    }
}

// Some FULL or ROOT value of the table matches the name (hyobfs_acl.h, "THE INDEX"): the whole
// name and every suffix that begins right after a '.' are looked up, the shortest first.
HY_HD bool index_lookup(const Slot* slots, uint32_t mask, const uint8_t* pats, const uint8_t* name, uint32_t nl) {
    if (nl == 0) return index_probe(slots, mask, pats, name, 0, 0, ix_mix(kIxBasis));
    uint32_t h = kIxBasis, c = name[nl - 1];
    for (uint32_t i = nl; i-- > 0;) {
        const uint32_t before = i ? name[i - 1] : '.';
        h = ix_step(h, c);
        if (before == '.' && index_probe(slots, mask, pats, name, i, nl, ix_mix(h))) return true;
        c = before;
    }
    return false;
}

// One entry against one item: compiledRule.Match (compile.go:62-70).
// `nt`: the name's last 16 bytes, the last one first, zero past its start.
// IDX: the rule set has a kDomainIndex entry (a set without one runs the code without that case).
template <bool IDX>
HY_HD bool entry_matches(const Entry& e, const Args& a, const uint8_t* name, uint32_t nl, const uint32_t* nt,
                         const Host& h, uint32_t proto, uint32_t port) {
    if (e.proto != 0 && e.proto != proto) return false;
    if (e.start_port != 0 && (port < e.start_port || port > e.end_port)) return false;
    const uint32_t pl = e.len;
    switch (e.kind) {
        case kAll:
            return true;
        case kIp: {
            const uint32_t* w = a.words + e.off;
            const uint32_t x[4] = {w[0], w[1], w[2], w[3]};
            return (h.has_a && prefix_eq(x, h.a, 128)) || (h.has_b && prefix_eq(x, h.b, 128));
        }
        case kCidr4:
        case kCidr6: {
            const bool is4 = e.kind == kCidr4;
            const uint32_t* w = a.words + e.off;
            const uint32_t x[4] = {w[0], w[1], w[2], w[3]};
            return (h.has_a && is4 && prefix_eq(x, h.a, pl)) || (h.has_b && h.b4 == is4 && prefix_eq(x, h.b, pl));
        }
        case kExact:
        case kSuffix: {
            // the lengths and the last 16 bytes from registers; the '.' before a suffix from LDS;
            // only a pattern longer than 16 bytes that agrees so far is read from memory
            if (e.kind == kExact ? pl != nl : pl > nl) return false;
            if (!tail_eq(nt, e.tail, pl < kTail ? pl : kTail)) return false;
            if (nl > pl && name[nl - pl - 1] != '.') return false;
            return pl <= kTail || bytes_eq(name, nl - pl, a.pats + e.off, pl - kTail);
        }
        case kWildcard:
            // whatever the stars take, the name is no shorter than the literals and ends as the pattern does
            if (nl < (e.tail[3] & 0xFFFF) || !tail_eq(nt, e.tail, e.tail[3] >> 16)) return false;
            return wildcard(name, nl, a.pats + e.off, pl);
        case kPlain: {
            if (pl > nl) return false;
            const uint32_t head = pl < kPlainHead ? pl : kPlainHead;
            for (uint32_t at = 0; at + pl <= nl; ++at) {
                bool eq = true;
#pragma unroll
                for (uint32_t k = 0; k < kPlainHead; ++k)
                    if (k < head) eq &= name[at + k] == ((e.tail[0] >> (8 * k)) & 0xFF);
                if (eq && (pl <= kPlainHead || bytes_eq(name, at + kPlainHead, a.pats + e.off + kPlainHead, pl - kPlainHead)))
                    return true;
            }
            return false;
        }
        case kCidrSet: {
            const uint32_t* s = a.words + e.off;
            bool found = h.has_a && cidr_set_has(s, h.a, true);
            if (!found && h.has_b) found = cidr_set_has(s, h.b, h.b4);
            return found != (s[2] != 0);
        }
        case kRegex:
            return rx::walk(a.dfa + e.off, e.tail[0], name, nl);
        case kDomainIndex:
            return IDX && index_lookup(a.slots + e.off, e.tail[0], a.pats, name, nl);
        default:
            return false;
    }
}

template <int MODE, bool IDX>
__global__ __launch_bounds__(64 * kWaves) void acl_kernel(Args a) {
    __shared__ uint8_t name_all[kWaves][kNameLds];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* name = name_all[wave];
    for (uint64_t m = (uint64_t)blockIdx.x * kWaves + wave; m < a.n; m += (uint64_t)gridDim.x * kWaves) {
        hyobfs_acl_result out{HYOBFS_OK, -1, 0, HYOBFS_ACL_NO_HIJACK};
        const uint8_t* p;
        uint32_t L;
        if (MODE == kSniffed) {
            const int st = __builtin_amdgcn_readfirstlane(a.sres[m].status);
            L = (uint32_t)__builtin_amdgcn_readfirstlane(a.sres[m].name_len);
            if (st != HYOBFS_OK || L == 0) {   // nothing of the name row is read
                out.status = HYOBFS_ACL_ERR_NO_NAME;
                if (lane == 0) a.res[m] = out;
                continue;
            }
            p = a.names + m * a.name_stride;
        } else {
            L = (uint32_t)__builtin_amdgcn_readfirstlane(a.name_len[m]);
            p = a.names + a.name_off[m];
        }
        if (L > HYOBFS_ACL_MAX_NAME) {
            out.status = HYOBFS_ACL_ERR_HOST;
            if (lane == 0) a.res[m] = out;
            continue;
        }
        // the name, a byte per lane and round, lower-cased (compile.go:89)
        uint32_t c[kNameLds / 64];
        bool host = false;
#pragma unroll
        for (uint32_t k = 0; k < kNameLds / 64; ++k) {
            const uint32_t i = lane + 64 * k;
            c[k] = i < L ? p[i] : 0;
            host |= c[k] >= 0x80;
            if (c[k] >= 'A' && c[k] <= 'Z') c[k] += 'a' - 'A';
        }
        hy_wave_sync();   // every lane's reads of the name staged before are done
#pragma unroll
        for (uint32_t k = 0; k < kNameLds / 64; ++k) name[lane + 64 * k] = (uint8_t)c[k];
        hy_wave_sync();
        // the length without trailing dots: one past the last byte that is not '.'
        uint32_t nl = 0;
#pragma unroll
        for (uint32_t k = kNameLds / 64; k-- > 0;) {
            const unsigned long long b = __ballot(lane + 64 * k < L && c[k] != '.');
            if (nl == 0 && b) nl = 64 * k + 64 - (uint32_t)__builtin_clzll(b);
        }
        // "xn--" anywhere: ToUnicode might rewrite the name (hyobfs_acl.h, fact 1)
#pragma unroll
        for (uint32_t k = 0; k < kNameLds / 64; ++k) {
            const uint32_t i = lane + 64 * k;
            if (i + 4 <= nl) host |= name[i] == 'x' && name[i + 1] == 'n' && name[i + 2] == '-' && name[i + 3] == '-';
        }
        if (__ballot(host)) {
            out.status = HYOBFS_ACL_ERR_HOST;
            if (lane == 0) a.res[m] = out;
            continue;
        }
        // the name's last 16 bytes for the entries' inline pieces (the same LDS bytes in every lane)
        uint32_t nt[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kTail; ++k)
            if (k < nl) nt[k / 4] |= (uint32_t)name[nl - 1 - k] << (8 * (k % 4));
        Host h{};
        const uint32_t fl = a.ip_flags ? a.ip_flags[m] : 0;
        if (fl & 1) {
            h.has_a = true;
            h.a[2] = 0xFFFF;
            h.a[3] = be32(a.ipv4 + 4 * m);
        }
        if (fl & 2) {
            h.has_b = true;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) h.b[w] = be32(a.ipv6 + 16 * m + 4 * w);
            h.b4 = h.b[0] == 0 && h.b[1] == 0 && h.b[2] == 0xFFFF;
        }
        const uint32_t proto = a.proto[m], port = a.port[m];
        // the walk: 64 entries per step, the first step with a hit decides
        int32_t rule = -1;
        for (uint32_t base = 0; base < a.n_entries; base += 64) {
            const uint32_t idx = base + lane;
            Entry e{};
            bool hit = false;
            if (idx < a.n_entries) {
                e = a.entries[idx];
                hit = entry_matches<IDX>(e, a, name, nl, nt, h, proto, port);
            }
            const unsigned long long b = __ballot(hit);
            if (b) {
                rule = __shfl((int)e.rule, (int)__builtin_ctzll(b));
                break;
            }
        }
        if (rule >= 0) {
            out.rule = rule;
            out.outbound = a.rule_out[rule].outbound;
            out.hijack = a.rule_out[rule].hijack;
        }
        if (lane == 0) a.res[m] = out;
    }
}

inline uint32_t grid_for(uint64_t n) {
    const uint64_t g = (n + kWaves - 1) / kWaves;
    return (uint32_t)(g < kGridCap ? g : kGridCap);
}

// `indexed`: the rule set has a kDomainIndex entry; every other set runs the kernel without that case
template <int MODE>
inline int launch(const Args& a, bool indexed, void* stream) {
    if (indexed)
        hipLaunchKernelGGL((acl_kernel<MODE, true>), dim3(grid_for(a.n)), dim3(64 * kWaves), 0,
                           static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((acl_kernel<MODE, false>), dim3(grid_for(a.n)), dim3(64 * kWaves), 0,
                           static_cast<hipStream_t>(stream), a);
    return hy_status(hipGetLastError());
}

static_assert(sizeof(hyobfs_acl_result) == 16, "hyobfs_acl_result layout");
static_assert(sizeof(hyobfs_acl_rule) == 64 && sizeof(hyobfs_acl_domain) == 16 && sizeof(hyobfs_acl_cidr) == 20,
              "hyobfs_acl_rule layout");

// ---- rule set creation (host)
struct Tables {
    std::vector<Entry> entries;
    std::vector<RuleOut> rule_out;
    std::vector<uint32_t> words;
    std::vector<uint8_t> pats;
    std::vector<uint16_t> dfa;
    std::vector<Slot> slots;
    std::vector<hyobfs_acl_index_info> index;   // per rule; slots == 0: the rule has no index
};

thread_local int64_t t_bad_rule = -1, t_bad_entry = -1;

inline bool v4_mapped(const uint8_t* a) {
    static const uint8_t pre[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFF, 0xFF};
    return std::memcmp(a, pre, 12) == 0;
}

// the address as net.IP.To16 gives it, in big-endian words
inline void push_addr16(std::vector<uint32_t>& w, const uint8_t* addr, uint32_t family) {
    if (family == 4) {
        w.insert(w.end(), {0u, 0u, 0xFFFFu, be32(addr)});
    } else {
        for (int k = 0; k < 4; ++k) w.push_back(be32(addr + 4 * k));
    }
}

inline int add_pattern(Tables& t, Entry e, uint32_t kind, const uint8_t* p, uint32_t len) {
    if (len > HYOBFS_ACL_MAX_NAME) return HYOBFS_ACL_ERR_PATTERN;
    if (!p && len) return HYOBFS_ERR_INVALID;
    e.kind = (uint8_t)kind;
    e.off = (uint32_t)t.pats.size();
    e.len = (uint16_t)len;
    auto put = [&e](uint32_t k, uint8_t b) { e.tail[k / 4] |= (uint32_t)b << (8 * (k % 4)); };
    if (kind == kExact || kind == kSuffix) {
        for (uint32_t k = 0; k < len && k < kTail; ++k) put(k, p[len - 1 - k]);
    } else if (kind == kWildcard) {
        uint32_t stars = 0, lit = 0;   // lit: literal bytes after the last '*'
        for (uint32_t k = 0; k < len; ++k) {
            stars += p[k] == '*';
            lit = p[k] == '*' ? 0 : lit + 1;
        }
        if (lit > kWildTail) lit = kWildTail;
        for (uint32_t k = 0; k < lit; ++k) put(k, p[len - 1 - k]);
        e.tail[3] = (len - stars) | lit << 16;
    } else {
        for (uint32_t k = 0; k < len && k < kPlainHead; ++k) put(k, p[k]);
    }
    if (len) t.pats.insert(t.pats.end(), p, p + len);
    t.entries.push_back(e);
    return HYOBFS_OK;
}

// The table of an indexed set: `vals` are its FULL and ROOT values, each with its type bit, and
// `entry` is the set's kDomainIndex entry.  Duplicate values are merged (a value given as both
// types keeps both bits); the slot count is the power of two that leaves the table at most half
// full; the values go in in sorted order, so the table does not depend on the order given.
inline int add_index(Tables& t, size_t entry, std::vector<std::pair<std::string, uint32_t>>& vals,
                     hyobfs_acl_index_info& info) {
    std::sort(vals.begin(), vals.end());
    size_t n = 0;
    for (size_t k = 0; k < vals.size(); ++k) {
        if (n && vals[n - 1].first == vals[k].first) {
            vals[n - 1].second |= vals[k].second;
        } else {
            if (n != k) vals[n] = std::move(vals[k]);
            ++n;
        }
    }
    vals.resize(n);
    uint64_t slots = 2;
    while (slots < 2 * (uint64_t)n) slots <<= 1;
    if (t.slots.size() + slots > 0xFFFFFFFFull) return HYOBFS_ERR_INVALID;
    const uint32_t first = (uint32_t)t.slots.size(), mask = (uint32_t)slots - 1;
    t.slots.resize(first + slots);   // all empty
    uint32_t longest = 0;
    for (const auto& v : vals) {
        const auto* p = reinterpret_cast<const uint8_t*>(v.first.data());
        const uint32_t len = (uint32_t)v.first.size(), hash = ix_hash(p, len);
        uint32_t s = hash & mask, probes = 1;
        for (; t.slots[first + s].meta; ++probes) s = (s - 1) & mask;
        t.slots[first + s] = Slot{hash, (uint32_t)t.pats.size(), len | v.second | kIxUsed, 0};
        t.pats.insert(t.pats.end(), p, p + len);
        longest = std::max(longest, probes);
    }
    t.entries[entry].off = first;
    t.entries[entry].tail[0] = mask;
    info = hyobfs_acl_index_info{(uint32_t)n, (uint32_t)slots, longest, 0};
    return HYOBFS_OK;
}

// One compiledRule into the tables; a status other than OK refuses the rule.  `index_min`: a
// DOMAIN_SET with at least this many FULL + ROOT entries is indexed; 0: none is.
int add_rule(Tables& t, const hyobfs_acl_rule& r, uint32_t index, uint32_t flags, uint32_t index_min) {
    if (r.kind > HYOBFS_ACL_CIDR_SET || r.proto > 2) return HYOBFS_ERR_INVALID;
    t.rule_out.push_back(RuleOut{r.outbound, r.hijack});
    t.index.push_back(hyobfs_acl_index_info{0, 0, 0, 0});
    Entry e{};
    e.rule = index;
    e.proto = (uint8_t)r.proto;
    e.start_port = r.start_port;
    e.end_port = r.end_port;
    switch (r.kind) {
        case HYOBFS_ACL_ALL:
            e.kind = kAll;
            t.entries.push_back(e);
            return HYOBFS_OK;
        case HYOBFS_ACL_IP:
        case HYOBFS_ACL_CIDR: {
            if (r.family != 4 && r.family != 6) return HYOBFS_ERR_INVALID;
            e.off = (uint32_t)t.words.size();
            if (r.kind == HYOBFS_ACL_IP) {
                e.kind = kIp;
            } else if (r.family == 4) {
                if (r.prefix > 32) return HYOBFS_ERR_INVALID;
                e.kind = kCidr4;
                e.len = (uint16_t)(96 + r.prefix);
            } else {
                if (r.prefix > 128) return HYOBFS_ERR_INVALID;
                // trap 3: a v4-mapped network is reduced to 4 bytes and the last four mask bytes
                const bool m4 = v4_mapped(r.addr);
                e.kind = m4 ? kCidr4 : kCidr6;
                e.len = (uint16_t)(m4 ? (r.prefix > 96 ? r.prefix : 96) : r.prefix);
            }
            push_addr16(t.words, r.addr, r.family);
            t.entries.push_back(e);
            return HYOBFS_OK;
        }
        case HYOBFS_ACL_DOMAIN_EXACT:
        case HYOBFS_ACL_DOMAIN_WILDCARD:
        case HYOBFS_ACL_DOMAIN_SUFFIX:
            if (!r.pattern) return HYOBFS_ERR_INVALID;
            return add_pattern(t, e,
                               r.kind == HYOBFS_ACL_DOMAIN_EXACT ? kExact
                                                                 : r.kind == HYOBFS_ACL_DOMAIN_WILDCARD ? kWildcard : kSuffix,
                               r.pattern, r.pattern_len);
        case HYOBFS_ACL_DOMAIN_SET: {
            if (!r.entries && r.n_entries) return HYOBFS_ERR_INVALID;
            const auto* d = static_cast<const hyobfs_acl_domain*>(r.entries);
            // indexed: its FULL and ROOT values are one kDomainIndex entry at the rule's position
            // and leave the walk; the count is of the entries as given, duplicates included
            bool indexed = false;
            if (index_min) {
                uint64_t fr = 0;
                for (uint32_t k = 0; k < r.n_entries; ++k)
                    fr += d[k].type == HYOBFS_ACL_DOMAIN_ROOT || d[k].type == HYOBFS_ACL_DOMAIN_FULL;
                indexed = fr >= index_min;
            }
            const size_t at = t.entries.size();
            std::vector<std::pair<std::string, uint32_t>> vals;
            if (indexed) {
                Entry x = e;
                x.kind = kDomainIndex;
                t.entries.push_back(x);
            }
            // the regex entries after the others (the set's result does not depend on the order)
            std::vector<Entry> regexes;
            for (uint32_t k = 0; k < r.n_entries; ++k) {
                t_bad_entry = k;
                if (indexed && (d[k].type == HYOBFS_ACL_DOMAIN_ROOT || d[k].type == HYOBFS_ACL_DOMAIN_FULL)) {
                    if (d[k].len > HYOBFS_ACL_MAX_NAME) return HYOBFS_ACL_ERR_PATTERN;
                    if (!d[k].value && d[k].len) return HYOBFS_ERR_INVALID;
                    vals.emplace_back(d[k].len ? std::string(reinterpret_cast<const char*>(d[k].value), d[k].len)
                                               : std::string(),
                                      d[k].type == HYOBFS_ACL_DOMAIN_FULL ? kIxFull : kIxRoot);
                    continue;
                }
                if (d[k].type == HYOBFS_ACL_DOMAIN_REGEX) {
                    if (!(flags & HYOBFS_ACL_FLAG_REGEX)) return HYOBFS_ACL_ERR_REGEX;
                    if (d[k].len > HYOBFS_ACL_MAX_NAME) return HYOBFS_ACL_ERR_PATTERN;
                    if (!d[k].value && d[k].len) return HYOBFS_ERR_INVALID;
                    rx::Dfa dfa;
                    if (!rx::compile(d[k].value, d[k].len, dfa)) return HYOBFS_ACL_ERR_REGEX;
                    if (t.dfa.size() + dfa.cells.size() > 0xFFFFFFFFull) return HYOBFS_ERR_INVALID;
                    Entry x = e;
                    x.kind = kRegex;
                    x.off = (uint32_t)t.dfa.size();
                    x.tail[0] = dfa.start;
                    t.dfa.insert(t.dfa.end(), dfa.cells.begin(), dfa.cells.end());
                    regexes.push_back(x);
                    continue;
                }
                if (d[k].type > HYOBFS_ACL_DOMAIN_FULL) return HYOBFS_ERR_INVALID;
                const int st = add_pattern(t, e,
                                           d[k].type == HYOBFS_ACL_DOMAIN_FULL ? kExact
                                                                               : d[k].type == HYOBFS_ACL_DOMAIN_ROOT ? kSuffix : kPlain,
                                           d[k].value, d[k].len);
                if (st != HYOBFS_OK) return st;
            }
            t_bad_entry = -1;
            t.entries.insert(t.entries.end(), regexes.begin(), regexes.end());
            return indexed ? add_index(t, at, vals, t.index[index]) : HYOBFS_OK;
        }
        default: {   // HYOBFS_ACL_CIDR_SET
            if (!r.entries && r.n_entries) return HYOBFS_ERR_INVALID;
            const auto* c = static_cast<const hyobfs_acl_cidr*>(r.entries);
            std::vector<const hyobfs_acl_cidr*> n4, n6;
            for (uint32_t k = 0; k < r.n_entries; ++k) {
                if (c[k].family == 4 && c[k].prefix <= 32) n4.push_back(&c[k]);
                else if (c[k].family == 6 && c[k].prefix <= 128) n6.push_back(&c[k]);
                else return HYOBFS_ERR_INVALID;
            }
            // by address bytes as given; stable, the shorter prefix first among equal addresses
            // (the reference's sort.Slice leaves their order open: hyobfs_acl.h)
            auto by_addr = [](size_t len) {
                return [len](const hyobfs_acl_cidr* x, const hyobfs_acl_cidr* y) {
                    const int cmp = std::memcmp(x->addr, y->addr, len);
                    return cmp != 0 ? cmp < 0 : x->prefix < y->prefix;
                };
            };
            std::stable_sort(n4.begin(), n4.end(), by_addr(4));
            std::stable_sort(n6.begin(), n6.end(), by_addr(16));
            e.kind = kCidrSet;
            e.off = (uint32_t)t.words.size();
            t.words.insert(t.words.end(), {(uint32_t)n4.size(), (uint32_t)n6.size(), r.inverse ? 1u : 0u, 0u});
            for (const auto* x : n4) t.words.insert(t.words.end(), {be32(x->addr), (uint32_t)x->prefix});
            for (const auto* x : n6) {
                for (int k = 0; k < 4; ++k) t.words.push_back(be32(x->addr + 4 * k));
                t.words.push_back(x->prefix | (v4_mapped(x->addr) ? 1u << 8 : 0u));
            }
            t.entries.push_back(e);
            return HYOBFS_OK;
        }
    }
}

inline uint64_t up16(uint64_t x) { return (x + 15) / 16 * 16; }

}  // namespace acl
}  // namespace hyobfs

using namespace hyobfs::acl;

struct hyobfs_acl_ruleset {
    int device = 0;
    uint32_t n_rules = 0, n_entries = 0;
    uint8_t* mem = nullptr;   // entries | rule_out | words | pats | dfa | slots, each from a 16-byte boundary
    const Entry* entries = nullptr;
    const RuleOut* rule_out = nullptr;
    const uint32_t* words = nullptr;
    const uint8_t* pats = nullptr;
    const uint16_t* dfa = nullptr;
    const Slot* slots = nullptr;
    bool indexed = false;                       // some rule has an index: the kernel with that case runs
    std::vector<hyobfs_acl_index_info> index;   // per rule
};

// The three creation calls.  `index_min` 0: no set is indexed.
static int ruleset_make(const hyobfs_acl_rule* rules, uint32_t n_rules, int device, uint32_t flags, uint32_t index_min,
                        hyobfs_acl_ruleset** out) {
    Tables t;
    for (uint32_t i = 0; i < n_rules; ++i) {
        const int st = add_rule(t, rules[i], i, flags, index_min);
        if (st != HYOBFS_OK) {
            t_bad_rule = i;
            return st;
        }
    }
    if (t.entries.size() > 0xFFFFFFFFull || t.words.size() > 0xFFFFFFFFull || t.pats.size() > 0xFFFFFFFFull)
        return HYOBFS_ERR_INVALID;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return HYOBFS_ERR_NO_DEVICE;
    auto* s = new (std::nothrow) hyobfs_acl_ruleset();
    if (!s) return HYOBFS_ERR_NOMEM;
    const uint64_t b_ent = up16(t.entries.size() * sizeof(Entry)), b_out = up16(t.rule_out.size() * sizeof(RuleOut)),
                   b_words = up16(t.words.size() * 4), b_pats = up16(t.pats.size()), b_dfa = up16(t.dfa.size() * 2),
                   b_slots = t.slots.size() * sizeof(Slot);
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    hipError_t e = hipSetDevice(device);
    void* mem = nullptr;
    if (e == hipSuccess) e = hipMalloc(&mem, b_ent + b_out + b_words + b_pats + b_dfa + b_slots + 16);
    uint8_t* d = static_cast<uint8_t*>(mem);
    if (e == hipSuccess && !t.entries.empty())
        e = hipMemcpy(d, t.entries.data(), t.entries.size() * sizeof(Entry), hipMemcpyHostToDevice);
    if (e == hipSuccess && !t.rule_out.empty())
        e = hipMemcpy(d + b_ent, t.rule_out.data(), t.rule_out.size() * sizeof(RuleOut), hipMemcpyHostToDevice);
    if (e == hipSuccess && !t.words.empty())
        e = hipMemcpy(d + b_ent + b_out, t.words.data(), t.words.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !t.pats.empty())
        e = hipMemcpy(d + b_ent + b_out + b_words, t.pats.data(), t.pats.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !t.dfa.empty())
        e = hipMemcpy(d + b_ent + b_out + b_words + b_pats, t.dfa.data(), t.dfa.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess && !t.slots.empty())
        e = hipMemcpy(d + b_ent + b_out + b_words + b_pats + b_dfa, t.slots.data(), b_slots, hipMemcpyHostToDevice);
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        delete s;
        return e == hipErrorOutOfMemory ? HYOBFS_ERR_NOMEM : HYOBFS_ERR_HIP;
    }
    s->device = device;
    s->n_rules = n_rules;
    s->n_entries = (uint32_t)t.entries.size();
    s->mem = d;
    s->entries = reinterpret_cast<const Entry*>(d);
    s->rule_out = reinterpret_cast<const RuleOut*>(d + b_ent);
    s->words = reinterpret_cast<const uint32_t*>(d + b_ent + b_out);
    s->pats = d + b_ent + b_out + b_words;
    s->dfa = reinterpret_cast<const uint16_t*>(d + b_ent + b_out + b_words + b_pats);
    s->slots = reinterpret_cast<const Slot*>(d + b_ent + b_out + b_words + b_pats + b_dfa);
    s->indexed = !t.slots.empty();
    s->index = std::move(t.index);
    *out = s;
    return HYOBFS_OK;
}

extern "C" {

int hyobfs_acl_ruleset_new(const hyobfs_acl_rule* rules, uint32_t n_rules, int device, hyobfs_acl_ruleset** out) {
    return hyobfs_acl_ruleset_new_flags(rules, n_rules, device, 0, out);
}

int hyobfs_acl_ruleset_new_flags(const hyobfs_acl_rule* rules, uint32_t n_rules, int device, uint32_t flags,
                                 hyobfs_acl_ruleset** out) {
    t_bad_rule = t_bad_entry = -1;
    if (!out || (!rules && n_rules) || (flags & ~HYOBFS_ACL_FLAG_REGEX)) return HYOBFS_ERR_INVALID;
    return ruleset_make(rules, n_rules, device, flags, 0, out);
}

int hyobfs_acl_ruleset_new_opts(const hyobfs_acl_rule* rules, uint32_t n_rules, int device,
                                const hyobfs_acl_options* opts, hyobfs_acl_ruleset** out) {
    if (!opts) return hyobfs_acl_ruleset_new(rules, n_rules, device, out);
    t_bad_rule = t_bad_entry = -1;
    if (!out || (!rules && n_rules)) return HYOBFS_ERR_INVALID;
    if (opts->struct_size != sizeof(hyobfs_acl_options) || opts->reserved != 0 ||
        (opts->flags & ~(HYOBFS_ACL_FLAG_REGEX | HYOBFS_ACL_FLAG_INDEX)))
        return HYOBFS_ERR_INVALID;
    const bool index = (opts->flags & HYOBFS_ACL_FLAG_INDEX) != 0;
    if (!index && opts->index_min != 0) return HYOBFS_ERR_INVALID;
    return ruleset_make(rules, n_rules, device, opts->flags & HYOBFS_ACL_FLAG_REGEX,
                        !index ? 0 : opts->index_min ? opts->index_min : HYOBFS_ACL_INDEX_MIN_DEFAULT, out);
}

void hyobfs_acl_ruleset_free(hyobfs_acl_ruleset* set) {
    if (!set) return;
    if (set->mem) (void)hipFree(set->mem);
    delete set;
}

uint32_t hyobfs_acl_ruleset_rules(const hyobfs_acl_ruleset* set) { return set ? set->n_rules : 0; }

uint32_t hyobfs_acl_ruleset_entries(const hyobfs_acl_ruleset* set) { return set ? set->n_entries : 0; }

int hyobfs_acl_ruleset_index_info(const hyobfs_acl_ruleset* set, uint32_t rule, hyobfs_acl_index_info* out) {
    if (!set || !out || rule >= set->n_rules) return HYOBFS_ERR_INVALID;
    *out = set->index[rule];
    return HYOBFS_OK;
}

int64_t hyobfs_acl_ruleset_bad_rule(void) { return t_bad_rule; }

int64_t hyobfs_acl_ruleset_bad_entry(void) { return t_bad_entry; }

int hyobfs_acl_regex_check(const uint8_t* pattern, uint32_t len, uint32_t* n_states, uint32_t* n_classes) {
    if (!pattern && len) return HYOBFS_ERR_INVALID;
    if (len > HYOBFS_ACL_MAX_NAME) return HYOBFS_ACL_ERR_PATTERN;
    rx::Dfa dfa;
    if (!rx::compile(pattern, len, dfa)) return HYOBFS_ACL_ERR_REGEX;
    if (n_states) *n_states = dfa.states;
    if (n_classes) *n_classes = dfa.classes;
    return HYOBFS_OK;
}

int hyobfs_acl_regex_match(const uint8_t* pattern, uint32_t len, const uint8_t* name, uint32_t name_len) {
    if ((!pattern && len) || (!name && name_len)) return HYOBFS_ERR_INVALID;
    if (len > HYOBFS_ACL_MAX_NAME) return HYOBFS_ACL_ERR_PATTERN;
    // this thread's last pattern stays compiled: one pattern is usually asked about many names
    thread_local std::vector<uint8_t> last;
    thread_local rx::Dfa dfa;
    thread_local bool have = false;
    if (!have || last.size() != len || !std::equal(last.begin(), last.end(), pattern)) {
        have = false;
        if (!rx::compile(pattern, len, dfa)) return HYOBFS_ACL_ERR_REGEX;
        last.assign(pattern, pattern + len);
        have = true;
    }
    return rx::walk(dfa.cells.data(), dfa.start, name, name_len) ? 1 : 0;
}

int hyobfs_acl_match_batch(const hyobfs_acl_ruleset* set, const uint8_t* names, const uint64_t* name_off,
                           const uint32_t* name_len, const uint8_t* ipv4, const uint8_t* ipv6, const uint8_t* ip_flags,
                           const uint8_t* proto, const uint16_t* port, uint64_t n, hyobfs_acl_result* res,
                           void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!set || !names || !name_off || !name_len || !proto || !port || !res || (ip_flags && (!ipv4 || !ipv6)))
        return HYOBFS_ERR_INVALID;
    return launch<kBatch>(Args{set->entries, set->rule_out, set->words, set->pats, set->dfa, set->slots, set->n_entries,
                               names, name_off, name_len, 0, nullptr, ipv4, ipv6, ip_flags, proto, port, n, res},
                          set->indexed, stream);
}

int hyobfs_acl_match_sniffed_batch(const hyobfs_acl_ruleset* set, const uint8_t* names, uint32_t name_stride,
                                   const hyobfs_sniff_result* sres, const uint8_t* ipv4, const uint8_t* ipv6,
                                   const uint8_t* ip_flags, const uint8_t* proto, const uint16_t* port, uint64_t n,
                                   hyobfs_acl_result* res, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!set || !names || !sres || !proto || !port || !res || (ip_flags && (!ipv4 || !ipv6))) return HYOBFS_ERR_INVALID;
    return launch<kSniffed>(Args{set->entries, set->rule_out, set->words, set->pats, set->dfa, set->slots, set->n_entries,
                                 names, nullptr, nullptr, name_stride, sres, ipv4, ipv6, ip_flags, proto, port, n, res},
                            set->indexed, stream);
}

}  // extern "C"
