// addr_rules.h -- rules H, P, I, T and F of include/hyobfs_addr.h, shared by the
// scalar host functions (addr_host.cpp, plain C++) and the device kernels
// (addr.hip, which defines HY_ADDR_FN as a device qualifier before including
// this).  Not installed.
//
// The parsers read their text through a byte source `s`: s(i) is byte i.  The
// host's is a pointer (PtrBytes), and so is the device's for a literal, over
// the LDS row that holds the text; for a port's digits the device reads the
// bytes a wave holds in its lanes' registers (addr.hip).
//
// A 16-byte address is two big-endian words here (hi = bytes 0-7, lo = bytes
// 8-15) and a group is picked out of them by shifts: no function keeps an
// array that is indexed at run time, so the device code needs no scratch.
#pragma once
#include <stdint.h>

#include "../../include/hyobfs_addr.h"

#ifndef HY_ADDR_FN
#define HY_ADDR_FN inline
#endif

namespace hyobfs {
namespace addr {

constexpr uint32_t kNone = 0xFFFFFFFFu;
typedef unsigned __int128 u128;

struct PtrBytes {
    const uint8_t* p;
    HY_ADDR_FN uint32_t operator()(uint32_t i) const { return p[i]; }
};

HY_ADDR_FN bool is_digit(uint32_t c) { return c - '0' < 10u; }
HY_ADDR_FN bool is_hex(uint32_t c) { return is_digit(c) || (c | 0x20) - 'a' < 6u; }
HY_ADDR_FN uint32_t hex_val(uint32_t c) { return is_digit(c) ? c - '0' : (c | 0x20) - 'a' + 10; }

// ---------------------------------------------------------------- rule H
// What net.SplitHostPort looks at: positions within the text, kNone for "none".
struct SplitFacts {
    uint32_t len;
    uint32_t first_colon, last_colon;
    uint32_t first_rb, last_rb;   // ']'
    bool lb0;                     // the text begins with '['
    bool lb_later;                // a '[' at index 1 or later
    bool colon_after_rb;          // text[first_rb + 1] == ':' (looked at only where it exists)
};
struct Split {
    int32_t status;
    uint32_t host_off, host_len, port_off, port_len;
};

HY_ADDR_FN Split split_fail(int32_t st) { return Split{st, 0, 0, 0, 0}; }

// net.SplitHostPort's decisions, in its order
HY_ADDR_FN Split split_decide(const SplitFacts& f) {
    if (f.last_colon == kNone) return split_fail(HYOBFS_ADDR_ERR_MISSING_PORT);   // H1
    const uint32_t i = f.last_colon;
    uint32_t h0 = 0, h1 = i;
    if (f.lb0) {
        const uint32_t end = f.first_rb;
        if (end == kNone) return split_fail(HYOBFS_ADDR_ERR_MISSING_BRACKET);
        if (end + 1 == f.len) return split_fail(HYOBFS_ADDR_ERR_MISSING_PORT);
        if (end + 1 != i)
            return split_fail(f.colon_after_rb ? HYOBFS_ADDR_ERR_TOO_MANY_COLONS : HYOBFS_ADDR_ERR_MISSING_PORT);
        h0 = 1;
        h1 = end;
        if (f.lb_later) return split_fail(HYOBFS_ADDR_ERR_UNEXPECTED_LBRACKET);                 // H2, j = 1
        if (f.last_rb != f.first_rb) return split_fail(HYOBFS_ADDR_ERR_UNEXPECTED_RBRACKET);    // H3, k = end + 1
    } else {
        if (f.first_colon != i) return split_fail(HYOBFS_ADDR_ERR_TOO_MANY_COLONS);
        if (f.lb_later) return split_fail(HYOBFS_ADDR_ERR_UNEXPECTED_LBRACKET);   // H2, j = 0: byte 0 is no '['
        if (f.first_rb != kNone) return split_fail(HYOBFS_ADDR_ERR_UNEXPECTED_RBRACKET);   // H3, k = 0
    }
    return Split{HYOBFS_OK, h0, h1 - h0, i + 1, f.len - i - 1};
}

// ---------------------------------------------------------------- rule P
// The value of a port's digits after its leading zeros: s(0 .. nsig - 1), all digits.
// More than five of them are more than 65535 whatever they are.
template <class S>
HY_ADDR_FN bool port_value(const S& s, uint32_t nsig, uint32_t* v) {
    *v = 0;
    if (nsig > 5) return false;
    uint32_t x = 0;
    for (uint32_t k = 0; k < nsig; ++k) x = x * 10 + (s(k) - '0');
    if (x > 65535) return false;
    *v = x;
    return true;
}

// ---------------------------------------------------------------- rule I
// parseIPv4Fields over s[off, end): the four fields as one big-endian word
template <class S>
HY_ADDR_FN bool parse_v4(const S& s, uint32_t off, uint32_t end, uint32_t* out) {
    uint32_t val = 0, pos = 0, dig = 0, acc = 0, prev = 0;
    for (uint32_t i = off; i < end; ++i) {
        const uint32_t c = s(i);
        if (is_digit(c)) {
            if (dig == 1 && val == 0) return false;   // a second digit after a leading '0'
            val = val * 10 + (c - '0');
            ++dig;
            if (val > 255) return false;
        } else if (c == '.') {
            if (i == off || i == end - 1 || prev == '.') return false;   // an empty field
            if (pos == 3) return false;                                  // a fifth field
            acc = acc << 8 | val;
            ++pos;
            val = 0;
            dig = 0;
        } else {
            return false;
        }
        prev = c;
    }
    if (pos < 3) return false;   // too few fields (the empty text included)
    *out = acc << 8 | val;
    return true;
}

// parseIPv6 over s[0, n), zones refused.  Groups are shifted into a 128-bit
// register; `ell` is the number of groups in front of the "::".
template <class S>
HY_ADDR_FN bool parse_v6(const S& s, uint32_t n, uint64_t* hi, uint64_t* lo) {
    uint64_t a_hi = 0, a_lo = 0;
    uint32_t ng = 0, ell = kNone, at = 0;
    auto push = [&](uint32_t g) {
        a_hi = a_hi << 16 | a_lo >> 48;
        a_lo = a_lo << 16 | g;
        ++ng;
    };
    if (n >= 2 && s(0) == ':' && s(1) == ':') {
        ell = 0;
        at = 2;
    }
    while (at < n && ng < 8) {
        uint32_t off = at, acc = 0;
        for (; off < n; ++off) {
            const uint32_t c = s(off);
            if (!is_hex(c)) break;
            if (off - at >= 4) return false;   // a fifth digit
            acc = acc << 4 | hex_val(c);
        }
        if (off == at) return false;   // a field without a digit
        if (off < n && s(off) == '.') {
            if (ell == kNone && ng != 6) return false;   // an embedded IPv4 replaces the final two fields
            if (ng + 2 > 8) return false;
            uint32_t v4;
            if (!parse_v4(s, at, n, &v4)) return false;
            push(v4 >> 16);
            push(v4 & 0xFFFF);
            at = n;
            break;
        }
        push(acc);
        at = off;
        if (at == n) break;
        if (s(at) != ':') return false;   // '%' included: a zone is refused
        if (at + 1 == n) return false;                           // a colon must be followed by more
        ++at;
        if (s(at) == ':') {
            if (ell != kNone) return false;   // a second "::"
            ell = ng;
            ++at;
            if (at == n) break;
        }
    }
    if (at != n) return false;   // bytes left over
    if (ng < 8) {
        if (ell == kNone) return false;   // too short
        // the groups behind the "::" stay at the low end, those in front move to the top
        const uint32_t tail = 16 * (ng - ell), sh = 16 * (8 - ell);   // tail <= 112, sh = 128 when nothing is in front
        const u128 a = (u128)a_hi << 64 | a_lo;
        const u128 t = tail ? a & (((u128)1 << tail) - 1) : (u128)0;
        const u128 h = sh >= 128 ? (u128)0 : (a >> tail) << sh;
        a_hi = (uint64_t)((h | t) >> 64);
        a_lo = (uint64_t)(h | t);
    } else if (ell != kNone) {
        return false;   // the "::" must stand for at least one zero group
    }
    *hi = a_hi;
    *lo = a_lo;
    return true;
}

// net.ParseIP over s[0, n): the 16-byte form
template <class S>
HY_ADDR_FN bool parse_ip(const S& s, uint32_t n, uint64_t* hi, uint64_t* lo) {
    *hi = *lo = 0;
    if (n > HYOBFS_ADDR_LITERAL_MAX) return false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = s(i);
        if (c == '.') {
            uint32_t v4;
            if (!parse_v4(s, 0, n, &v4)) return false;
            *lo = 0xFFFF00000000ull | v4;
            return true;
        }
        if (c == ':') {
            if (parse_v6(s, n, hi, lo)) return true;
            *hi = *lo = 0;
            return false;
        }
        if (c == '%') return false;
    }
    return false;
}

// ---------------------------------------------------------------- rule T
HY_ADDR_FN bool is_v4_mapped(uint64_t hi, uint64_t lo) { return hi == 0 && (lo >> 32) == 0xFFFFu; }   // To4() != nil

// ---------------------------------------------------------------- rule F
HY_ADDR_FN uint32_t put_dec(uint8_t* out, uint32_t at, uint32_t v) {   // v < 100000
    const uint32_t nd = v >= 10000 ? 5 : v >= 1000 ? 4 : v >= 100 ? 3 : v >= 10 ? 2 : 1;
    for (uint32_t k = nd; k-- > 0;) {
        out[at + k] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return at + nd;
}
HY_ADDR_FN uint32_t group_of(uint64_t hi, uint64_t lo, uint32_t g) {
    return (uint32_t)((g < 4 ? hi : lo) >> (48 - 16 * (g & 3))) & 0xFFFFu;
}

// The text of (ip, port) in out[0, HYOBFS_ADDR_FORMAT_MAX): its length, or
// HYOBFS_ADDR_ERR_FAMILY.  Family 4 takes the top four bytes of hi.
HY_ADDR_FN int format(uint64_t hi, uint64_t lo, uint32_t family, uint32_t port, uint8_t* out) {
    if (family != 4 && family != 16) return HYOBFS_ADDR_ERR_FAMILY;
    uint32_t at = 0;
    if (family == 4 || is_v4_mapped(hi, lo)) {
        const uint32_t v4 = family == 4 ? (uint32_t)(hi >> 32) : (uint32_t)lo;
        for (uint32_t k = 0; k < 4; ++k) {
            if (k) out[at++] = '.';
            at = put_dec(out, at, (v4 >> (24 - 8 * k)) & 0xFFu);
        }
    } else {
        uint32_t z0 = 8, z1 = 8;   // the longest run of two or more zero groups, the first on a tie
        for (uint32_t i = 0; i < 8; ++i) {
            uint32_t j = i;
            while (j < 8 && group_of(hi, lo, j) == 0) ++j;
            if (j - i >= 2 && j - i > z1 - z0) {
                z0 = i;
                z1 = j;
            }
        }
        out[at++] = '[';
        for (uint32_t i = 0; i < 8; ++i) {
            if (i == z0) {
                out[at++] = ':';
                out[at++] = ':';
                i = z1;
                if (i >= 8) break;
            } else if (i > 0) {
                out[at++] = ':';
            }
            const uint32_t g = group_of(hi, lo, i);
            const uint32_t nd = g >= 0x1000 ? 4 : g >= 0x100 ? 3 : g >= 0x10 ? 2 : 1;
            for (uint32_t k = 0; k < nd; ++k) {
                const uint32_t d = (g >> (4 * (nd - 1 - k))) & 0xFu;
                out[at++] = (uint8_t)(d < 10 ? '0' + d : 'a' + d - 10);
            }
        }
        out[at++] = ']';
    }
    out[at++] = ':';
    return (int)put_dec(out, at, port & 0xFFFFu);
}

}  // namespace addr
}  // namespace hyobfs
