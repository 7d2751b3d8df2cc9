// request_rules.h -- rules R, T, Q, S, G, C4-C5 and W of include/hyobfs_request.h,
// shared by the scalar host functions (request_host.cpp, plain C++) and the
// device kernels (request.hip, which defines HY_REQ_FN as a device qualifier
// before including this).  Rules H and I come from addr_rules.h and rule V's
// writing side from udpmsg_rules.h; neither is restated here.  Not installed.
//
// Texts are read through a byte source `s` (s(i) is byte i), as in addr_rules.h.
#pragma once
#include <stdint.h>

#include "../../include/hyobfs_request.h"

#ifndef HY_REQ_FN
#define HY_REQ_FN inline
#endif
#ifndef HY_ADDR_FN
#define HY_ADDR_FN HY_REQ_FN
#endif
#ifndef HY_UDP_FN
#define HY_UDP_FN HY_REQ_FN
#endif
#include "addr_rules.h"
#include "udpmsg_rules.h"

namespace hyobfs {
namespace request {

using addr::kNone;
using udpmsg::varint_byte;
using udpmsg::varint_len;

// ---------------------------------------------------------------- rule V, reading
HY_REQ_FN uint32_t varint_size(uint32_t b0) { return 1u << (b0 >> 6); }
template <class S>
HY_REQ_FN uint64_t varint_get(const S& s, uint32_t at, uint32_t vl) {
    uint64_t v = s(at) & 0x3Fu;
    for (uint32_t k = 1; k < vl; ++k) v = v << 8 | s(at + k);
    return v;
}

// ---------------------------------------------------------------- rules R and T
// A status byte or none (`lead`), a length-prefixed text, a length-prefixed padding.
struct Framed {
    int32_t status;
    uint32_t need;       // NEED_MORE only
    uint32_t text_off, text_len;
    uint32_t consumed;
};
HY_REQ_FN Framed framed_fail(int32_t st, uint64_t need) { return Framed{st, (uint32_t)need, 0, 0, 0}; }

// lead == 0: ReadTCPRequest (the text is the address, 1..2048 bytes); lead == 1: ReadTCPResponse (the text is the
// message, 0..2048 bytes).  Every position below is at most 1 + 8 + 2048 + 8 + 4096.
template <class S>
HY_REQ_FN Framed parse_framed(const S& s, uint64_t len, uint32_t lead) {
    if (len < lead) return framed_fail(HYOBFS_REQ_ERR_NEED_MORE, lead);                              // T: no status byte
    if (len < lead + 1) return framed_fail(HYOBFS_REQ_ERR_NEED_MORE, lead + 1);                      // R1
    const uint32_t vl = varint_size(s(lead));
    if (len < lead + vl) return framed_fail(HYOBFS_REQ_ERR_NEED_MORE, lead + vl);
    const uint64_t v = varint_get(s, lead, vl);
    if (lead == 0 ? (v == 0 || v > HYOBFS_REQ_MAX_ADDR) : v > HYOBFS_REQ_MAX_MSG)                       // R2
        return framed_fail(lead == 0 ? HYOBFS_REQ_ERR_ADDR_LEN : HYOBFS_REQ_ERR_MSG_LEN, 0);
    const uint32_t t0 = lead + vl, t1 = t0 + (uint32_t)v;
    if (len < t1 + 1) return framed_fail(HYOBFS_REQ_ERR_NEED_MORE, t1 + 1);                          // R3
    const uint32_t vl2 = varint_size(s(t1));
    if (len < t1 + vl2) return framed_fail(HYOBFS_REQ_ERR_NEED_MORE, t1 + vl2);                      // R4
    const uint64_t p = varint_get(s, t1, vl2);
    if (p > HYOBFS_REQ_MAX_PADDING) return framed_fail(HYOBFS_REQ_ERR_PADDING_LEN, 0);                  // R5
    const uint32_t total = t1 + vl2 + (uint32_t)p;
    if (len < total) return framed_fail(HYOBFS_REQ_ERR_NEED_MORE, total);                            // R6
    return Framed{HYOBFS_OK, 0, t0, (uint32_t)v, total};
}

// ---------------------------------------------------------------- rule G
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
HY_REQ_FN uint64_t mix(uint64_t x) {   // SplitMix64's output function
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
HY_REQ_FN uint64_t pad_state(uint64_t seed, uint64_t item) { return mix(seed + kGolden * (item + 1)); }
HY_REQ_FN uint64_t pad_block(uint64_t state, uint64_t k) { return mix(state + kGolden * (k / 4 + 1)); }   // bytes 4 (k/4) ..+3
HY_REQ_FN uint8_t pad_char(uint32_t g) {   // paddingChars[g % 62]
    const uint32_t r = g % 62u;
    return (uint8_t)(r < 26 ? 'a' + r : r < 52 ? 'A' + (r - 26) : '0' + (r - 52));
}
HY_REQ_FN uint8_t pad_byte(uint64_t state, uint64_t k) {
    return pad_char((uint32_t)(pad_block(state, k) >> (16 * (k & 3))) & 0xFFFFu);
}

// ---------------------------------------------------------------- rules Q and S
// Where the parts of a written frame lie: head (the frame type or the status byte, and the text's length), the
// text, the padding's length, the padding.
struct FrameLayout {
    uint32_t lead_len;            // bytes in front of the text's length: 2 (the 0x401 varint) or 1 (the status)
    uint32_t vl_text, vl_pad;
    uint64_t text_len, pad_len;
    HY_REQ_FN uint64_t text_at() const { return lead_len + vl_text; }
    HY_REQ_FN uint64_t padlen_at() const { return text_at() + text_len; }
    HY_REQ_FN uint64_t pad_at() const { return padlen_at() + vl_pad; }
    HY_REQ_FN uint64_t total() const { return pad_at() + pad_len; }
};
HY_REQ_FN FrameLayout frame_layout(uint32_t lead_len, uint64_t text_len, uint64_t pad_len) {
    return FrameLayout{lead_len, varint_len(text_len), varint_len(pad_len), text_len, pad_len};
}

// ---------------------------------------------------------------- rules C4 and C5
HY_REQ_FN bool is_sign(uint32_t c) { return c == '+' || c == '-'; }

// strconv.Atoi's value as a uint16: s(0 .. nsig - 1) are the digits behind the sign and the leading zeros.
// false: out of [-2^63, 2^63 - 1] (ErrRange).  Nineteen digits fit a uint64; twenty never fit an int64.
template <class S>
HY_REQ_FN bool atoi_port16(const S& s, uint32_t nsig, bool neg, uint32_t* port16) {
    *port16 = 0;
    if (nsig > 19) return false;
    uint64_t m = 0;
    for (uint32_t k = 0; k < nsig; ++k) m = m * 10 + (s(k) - '0');
    if (m > (neg ? 1ull << 63 : (1ull << 63) - 1)) return false;
    *port16 = (uint32_t)(neg ? 0 - m : m) & 0xFFFFu;
    return true;
}

// ---------------------------------------------------------------- rule W
enum RewriteMode { kCopy = 0, kJoin = 1, kLeftToHost = 2 };
HY_REQ_FN RewriteMode rewrite_mode(bool check, int32_t sniff_status, uint32_t name_len) {
    if (!check) return kCopy;                                                       // W1
    if (sniff_status == HYOBFS_OK) return name_len ? kJoin : kCopy;                  // W2
    if (sniff_status == HYOBFS_SNIFF_ERR_NEED_MORE || sniff_status == HYOBFS_SNIFF_ERR_HOST ||
        sniff_status == HYOBFS_SNIFF_ERR_NAME_CAP)
        return kLeftToHost;
    return kCopy;
}
HY_REQ_FN bool needs_brackets(uint32_t c) { return c == ':' || c == '%'; }   // net.JoinHostPort

}  // namespace request
}  // namespace hyobfs
