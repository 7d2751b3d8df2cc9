// sniff_http.h -- the HTTP branch of the sniffer (include/hyobfs_sniff.h, rules
// H0-H7): the host part of the Host header of a request's first bytes.
//
// Reference: apernet/hysteria extras/sniff/sniff.go (isHTTP :46-57, the HTTP
// branch of TCP :110-127) and the rules of Go's http.ReadRequest that the
// header restates.
//
// One WAVE parses one request.  Unlike a ClientHello, a header block has no
// length prefixes, so the walk is a scan: the wave stages kHttpStage bytes in
// LDS with coalesced loads, then takes them 64 at a time, a byte per lane.
// Each lane classifies its byte, ballots turn the classes into 64-bit masks,
// and wave-uniform bit operations on the masks find the line ends and the
// first colon of each line and test "every key byte legal" and "every value
// byte legal".  What a line needs beyond that (its start, its colon, whether a
// bad byte was seen, a CR that ended the step before) is carried in
// wave-uniform scalars, so a line may straddle any number of steps.  The rare
// work is done when its line ends and reads the bytes again, from LDS where
// they are still staged (a request of up to kHttpStage bytes always is) and
// from memory otherwise: the request line's three fields, a header name (only
// for keys of 4, 7, 14 or 17 bytes), and after the block the Host and
// Content-Length values.
//
// Every function here is wave-uniform: all 64 lanes call it with the same
// arguments apart from `lane` and get the same result.  A byte that every lane
// loads for itself and that decides a branch goes through readfirstlane (uni),
// so the compiler keeps the walk's state and its branches scalar.
#pragma once
#include "kernels.h"
#include "../../include/hyobfs_sniff.h"

namespace hyobfs {
namespace sniff {

constexpr uint32_t kHttpMax = 256 * 1024;   // sniffMaxHTTPHeaderBytes, sniff.go:21
constexpr uint32_t kHttpStage = 1024;       // bytes a wave stages in LDS at a time
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct HttpParsed {
    int status;
    uint32_t name_off, name_len, need;
};

constexpr uint32_t tchar_word(int w) {   // RFC 7230 tchar, bytes [32 w, 32 w + 32)
    const char s[] = "!#$%&'*+-.^_`|~0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz";
    uint32_t v = 0;
    for (int i = 0; s[i]; ++i)
        if ((s[i] >> 5) == w) v |= 1u << (s[i] & 31);
    return v;
}
__device__ inline bool is_tchar(uint32_t c) {
    constexpr uint32_t w1 = tchar_word(1), w2 = tchar_word(2), w3 = tchar_word(3);
    const uint32_t w = c < 64 ? (c < 32 ? 0u : w1) : c < 96 ? w2 : c < 128 ? w3 : 0u;
    return (w >> (c & 31)) & 1;
}
__device__ inline bool is_alpha(uint32_t c) { return (c | 0x20) - 'a' < 26u; }
__device__ inline bool is_digit(uint32_t c) { return c - '0' < 10u; }
__device__ inline bool is_hex(uint32_t c) { return is_digit(c) || (c | 0x20) - 'a' < 6u; }
__device__ inline bool is_ws(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
// The bytes of one stream: those staged in LDS, and memory for the rest.
struct HttpBytes {
    const uint8_t* p;
    const uint8_t* lds;
    uint32_t base, limit;   // lds holds p[base, base + limit)
    __device__ uint32_t operator[](uint32_t i) const { return i - base < limit ? lds[i - base] : p[i]; }
};

// Byte i (< 24) of a string of up to 24 bytes held in three constants, so that a lane's
// byte of a header name comes from registers, not from a load of constant memory.
constexpr uint64_t str_word(const char* s, int w) {
    uint64_t v = 0;
    int n = 0;
    while (s[n]) ++n;
    for (int i = 8 * w; i < 8 * w + 8 && i < n; ++i) v |= (uint64_t)(uint8_t)s[i] << (8 * (i - 8 * w));
    return v;
}
template <uint64_t W0, uint64_t W1, uint64_t W2>
__device__ inline uint32_t str_byte(uint32_t i) {
    return (uint32_t)((i < 8 ? W0 : i < 16 ? W1 : W2) >> (8 * (i & 7))) & 0xFF;
}
#define HY_STR_BYTE(s, i) (str_byte<str_word(s, 0), str_word(s, 1), str_word(s, 2)>(i))

__device__ inline uint64_t bits_below(uint32_t b) { return b < 64 ? ~(~0ull << b) : ~0ull; }   // bits [0, b)

// H1-H4 over the request line p[0, cend); p[cend] is its CR or LF.
__device__ inline int http_request_line(const HttpBytes& p, uint32_t cend, uint32_t lane) {
    uint32_t sp1 = kNone, sp2 = kNone, query = kNone, want_hex = 0;
    bool method_bad = false, ctl = false, pct_bad = false;
    for (uint32_t pos = 0; pos < cend; pos += 64) {
        const uint32_t idx = pos + lane;
        const bool in = idx < cend;
        const uint32_t c = in ? p[idx] : 0;
        uint64_t sp = __ballot(in && c == ' ');
        if (sp1 == kNone && sp) {
            sp1 = pos + __builtin_ctzll(sp);
            sp &= sp - 1;
        }
        if (sp1 != kNone && sp2 == kNone && sp) sp2 = pos + __builtin_ctzll(sp);
        method_bad |= __ballot(in && idx < sp1 && !is_tchar(c)) != 0;
        const bool uri = in && sp1 != kNone && idx > sp1 && idx < sp2;
        const uint64_t q = __ballot(uri && c == '?');
        if (query == kNone && q) query = pos + __builtin_ctzll(q);
        ctl |= __ballot(uri && (c < 0x20 || c == 0x7F)) != 0;
        // a '%' of the path wants a hex digit in each of the next two bytes (0 past the line's end)
        const uint64_t pct = __ballot(uri && idx < query && c == '%'), hex = __ballot(is_hex(c));
        pct_bad |= ((pct << 1 | pct << 2 | want_hex) & ~hex) != 0;
        want_hex = (uint32_t)(pct >> 63) * 3 | ((uint32_t)(pct >> 62) & 1);
    }
    if (sp1 == kNone || sp2 == kNone) return HYOBFS_SNIFF_ERR_MALFORMED;   // H1
    if (sp1 == 0 || method_bad) return HYOBFS_SNIFF_ERR_MALFORMED;         // H2
    bool proto_bad = false;                                                // H3
    if (cend - sp2 - 1 == 8 && lane < 8) {
        const uint32_t c = p[sp2 + 1 + lane];
        proto_bad = lane == 5 || lane == 7 ? !is_digit(c) : c != HY_STR_BYTE("HTTP/0.0", lane);
    }
    if (cend - sp2 - 1 != 8 || __ballot(proto_bad)) return HYOBFS_SNIFF_ERR_MALFORMED;
    if (sp2 - sp1 == 1) return HYOBFS_SNIFF_ERR_MALFORMED;                 // H4
    const uint32_t u0 = uni(p[sp1 + 1]);
    if (u0 == '*' && sp2 - sp1 == 2) return HYOBFS_OK;
    if (u0 != '/') return HYOBFS_SNIFF_ERR_HOST;
    return ctl || pct_bad || want_hex ? HYOBFS_SNIFF_ERR_MALFORMED : HYOBFS_OK;
}

enum HttpHeader { kHdrOther = 0, kHdrHost, kHdrContentLength, kHdrCoded };

// Which of the named headers the key p[ls, ls + klen) is, ASCII case-insensitively.
__device__ inline int http_header_name(const HttpBytes& p, uint32_t ls, uint32_t klen, uint32_t lane) {
    const uint32_t want = klen == 4 ? HY_STR_BYTE("host", lane) : klen == 7 ? HY_STR_BYTE("trailer", lane)
                          : klen == 14 ? HY_STR_BYTE("content-length", lane) : HY_STR_BYTE("transfer-encoding", lane);
    bool differs = false;
    if (lane < klen) {
        uint32_t c = p[ls + lane];
        if (c - 'A' < 26u) c |= 0x20;
        differs = c != want;
    }
    if (__ballot(differs)) return kHdrOther;
    return klen == 4 ? kHdrHost : klen == 14 ? kHdrContentLength : kHdrCoded;
}

// p[a, b) without its leading and trailing SP / HT.
__device__ inline void http_trim(const HttpBytes& p, uint32_t& a, uint32_t& b, uint32_t lane) {
    while (a < b) {
        const uint64_t keep = __ballot(lane < b - a && !is_ws(p[lane < b - a ? a + lane : a]));
        if (keep) {
            a += __builtin_ctzll(keep);
            break;
        }
        a = b - a > 64 ? a + 64 : b;
    }
    while (a < b) {
        const uint64_t keep = __ballot(lane < b - a && !is_ws(p[lane < b - a ? b - 1 - lane : a]));
        if (keep) {
            b -= __builtin_ctzll(keep);
            break;
        }
        b = b - a > 64 ? b - 64 : a;
    }
}

// H7 over the non-empty Host value p[a, b): net.SplitHostPort's host, the whole
// value on its error, HYOBFS_SNIFF_ERR_HOST for an empty host part.
__device__ inline HttpParsed http_host_part(const HttpBytes& p, uint32_t a, uint32_t b, uint32_t lane) {
    uint32_t first_colon = kNone, last_colon = kNone, first_rb = kNone, last_rb = kNone;
    bool lb_later = false;   // a '[' past the first byte
    for (uint32_t pos = a; pos < b; pos += 64) {
        const bool in = lane < b - pos;
        const uint32_t c = in ? p[pos + lane] : 0;
        const uint64_t colon = __ballot(c == ':'), rb = __ballot(c == ']');
        if (colon) {
            if (first_colon == kNone) first_colon = pos + __builtin_ctzll(colon);
            last_colon = pos + 63 - __builtin_clzll(colon);
        }
        if (rb) {
            if (first_rb == kNone) first_rb = pos + __builtin_ctzll(rb);
            last_rb = pos + 63 - __builtin_clzll(rb);
        }
        lb_later |= __ballot(c == '[' && pos + lane > a) != 0;
    }
    const HttpParsed whole{HYOBFS_OK, a, b - a, 0};
    if (last_colon == kNone) return whole;                      // missing port
    uint32_t h0 = a, h1 = last_colon;
    if (uni(p[a]) == '[') {
        if (first_rb == kNone || first_rb + 1 == b || first_rb + 1 != last_colon) return whole;
        if (lb_later || last_rb != first_rb) return whole;
        h0 = a + 1;
        h1 = first_rb;
    } else if (first_colon != last_colon || lb_later || first_rb != kNone) {
        return whole;                                            // too many colons, a stray bracket
    }
    if (h0 == h1) return HttpParsed{HYOBFS_SNIFF_ERR_HOST, 0, 0, 0};
    return HttpParsed{HYOBFS_OK, h0, h1 - h0, 0};
}

// Rules H0-H7 over p[0, len); `lds` is this wave's kHttpStage bytes.  name_off
// is relative to p.  NAME_CAP is the caller's.
__device__ inline HttpParsed http_parse(const uint8_t* msg, uint32_t len, uint8_t* lds, uint32_t lane) {
    const HttpParsed not_http{HYOBFS_SNIFF_ERR_NOT_HTTP, 0, 0, 0};
    if (len < 3) return not_http;                                           // H0
    HttpBytes p{msg, lds, 0, 0};
    const HttpParsed malformed{HYOBFS_SNIFF_ERR_MALFORMED, 0, 0, 0}, to_host{HYOBFS_SNIFF_ERR_HOST, 0, 0, 0};
    const uint32_t L = len < kHttpMax ? len : kHttpMax;
    // the line being read: 0 the request line, 1 the first header line, 2 a later one
    uint32_t phase = 0, ls = 0, colon = kNone;
    bool bad = false, first_ws = false, pend_cr = false;
    uint32_t hosts = 0, clens = 0, host_a = 0, host_b = 0, cl_a = 0, cl_b = 0;
    bool coded = false, ended = false;
    for (uint32_t base = 0; base < L && !ended; base += kHttpStage) {
        const uint32_t limit = L - base < kHttpStage ? L - base : kHttpStage;
        uint8_t v[kHttpStage / 64];
#pragma unroll
        for (uint32_t k = 0; k < kHttpStage / 64; ++k) v[k] = lane + 64 * k < limit ? msg[base + lane + 64 * k] : 0;
        hy_wave_sync();   // every lane's reads of the bytes staged before are done
#pragma unroll
        for (uint32_t k = 0; k < kHttpStage / 64; ++k) lds[lane + 64 * k] = v[k];
        hy_wave_sync();
        p.base = base;
        p.limit = limit;
        if (base == 0 && !(is_alpha(uni(p[0])) && is_alpha(uni(p[1])) && is_alpha(uni(p[2])))) return not_http;   // H0, isHTTP
        for (uint32_t pos = base; pos < base + limit && !ended; pos += 64) {
            const uint32_t c = lds[pos - base + lane];   // 0 past L
            const uint64_t lf = __ballot(c == '\n'), cr = __ballot(c == '\r'), col = __ballot(c == ':');
            const uint64_t ws = __ballot(is_ws(c));
            const uint64_t key_bad = __ballot(!(is_tchar(c) || c == ' '));
            const uint64_t val_bad = __ballot(!(c == '\t' || (c >= 0x20 && c != 0x7F)));
            // a CR that ended the step before belongs to the line's end only if this step begins with the LF
            const bool cr_carried = pend_cr && (lf & 1);
            if (pend_cr && !cr_carried) bad = true;
            pend_cr = false;
            uint32_t cur = 0;
            while (cur < 64) {
                const uint64_t from = ~0ull << cur, lfm = lf & from;
                const uint32_t e = lfm ? __builtin_ctzll(lfm) : 64;   // this line's bytes in the step: [cur, e)
                uint64_t seg = from & bits_below(e);
                bool stripped = e == 0 && cr_carried;
                if (e > cur && ((cr >> (e - 1)) & 1)) {                // one CR directly before the LF
                    seg &= ~(1ull << (e - 1));
                    if (e < 64) stripped = true;
                    else pend_cr = true;
                }
                if (phase != 0) {
                    if (ls == pos + cur) first_ws = (ws >> cur) & 1;
                    uint64_t key = 0, val = seg;
                    if (colon == kNone) {
                        const uint64_t cm = col & seg;
                        key = seg;
                        val = 0;
                        if (cm) {
                            const uint32_t b = __builtin_ctzll(cm);
                            colon = pos + b;
                            key = seg & bits_below(b);
                            val = seg & ~bits_below(b + 1);
                        }
                    }
                    bad |= ((key & key_bad) | (val & val_bad)) != 0;
                }
                if (e == 64) break;
                const uint32_t cend = pos + e - (stripped ? 1 : 0);    // the complete line is p[ls, cend)
                if (phase == 0) {
                    const int st = http_request_line(p, cend, lane);
                    if (st != HYOBFS_OK) return HttpParsed{st, 0, 0, 0};
                    phase = 1;
                } else {
                    if (cend == ls) {                                   // the blank line
                        ended = true;
                        break;
                    }
                    if (first_ws) return phase == 1 ? malformed : to_host;   // H5
                    if (bad || colon == kNone) return malformed;
                    const uint32_t klen = colon - ls;
                    if (klen == 4 || klen == 7 || klen == 14 || klen == 17) {
                        const int h = http_header_name(p, ls, klen, lane);
                        if (h == kHdrHost && hosts++ == 0) {
                            host_a = colon + 1;
                            host_b = cend;
                        } else if (h == kHdrContentLength && clens++ == 0) {
                            cl_a = colon + 1;
                            cl_b = cend;
                        } else if (h == kHdrCoded) {
                            coded = true;
                        }
                    }
                    phase = 2;
                }
                ls = pos + e + 1;
                colon = kNone;
                bad = first_ws = false;
                cur = e + 1;
            }
        }
    }
    if (!ended) {
        if (len >= kHttpMax) return malformed;
        return HttpParsed{HYOBFS_SNIFF_ERR_NEED_MORE, 0, 0, len + 1};
    }
    if (hosts > 1) return malformed;                                    // H6
    if (coded || clens > 1) return to_host;
    if (clens) {
        http_trim(p, cl_a, cl_b, lane);
        const uint32_t n = cl_b - cl_a;
        if (n < 1 || n > 18) return to_host;
        if (__ballot(lane < n && !is_digit(p[lane < n ? cl_a + lane : cl_a]))) return to_host;
    }
    if (hosts) http_trim(p, host_a, host_b, lane);
    if (!hosts || host_a == host_b) return HttpParsed{HYOBFS_OK, 0, 0, 0};
    return http_host_part(p, host_a, host_b, lane);
}

}  // namespace sniff
}  // namespace hyobfs
