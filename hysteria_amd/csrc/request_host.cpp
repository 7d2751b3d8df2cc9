// request_host.cpp -- host side of the request hook (include/hyobfs_request.h):
// ReadTCPRequest / WriteTCPRequest / ReadTCPResponse / WriteTCPResponse
// (core/internal/protocol/proxy.go:32-149), ParsePortUnion and Contains
// (extras/utils/portunion.go), Sniffer.Check and the address rewrite
// (extras/sniff/sniff.go:67-89, 121-125) for one item.  Plain host C++; the
// device batch calls live in request.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "request_rules.h"

using namespace hyobfs::request;
using hyobfs::addr::PtrBytes;

namespace {

// rules Q / S: the frame in out[0, cap), or -1
int64_t build(uint32_t lead_len, const uint8_t* lead, const uint8_t* text, size_t text_len, uint32_t pad_len, uint64_t seed,
              uint64_t item, uint8_t* out, size_t cap) {
    const FrameLayout f = frame_layout(lead_len, text_len, pad_len);
    if (f.total() > cap) return -1;
    memcpy(out, lead, lead_len);
    for (uint32_t k = 0; k < f.vl_text; ++k) out[lead_len + k] = varint_byte(text_len, f.vl_text, k);
    if (text_len) memcpy(out + f.text_at(), text, text_len);
    for (uint32_t k = 0; k < f.vl_pad; ++k) out[f.padlen_at() + k] = varint_byte(pad_len, f.vl_pad, k);
    hyobfs_req_padding_fill(seed, item, out + f.pad_at(), pad_len);
    return (int64_t)f.total();
}

bool contains(const hyobfs_port_range* r, int64_t n, uint16_t port) {   // rule K
    if (n < 0) return true;
    for (int64_t i = 0; i < n; ++i)
        if (port >= r[i].start && port <= r[i].end) return true;
    return false;
}

// rule U's numbers are rule P's (strconv.ParseUint(.., 10, 16))
bool parse_u16(const uint8_t* p, size_t n, uint16_t* v) { return hyobfs_addr_parse_port(n ? p : nullptr, n, v) == HYOBFS_OK; }

// rules C1-C5: the port Check looks up, or false
bool check_port(const uint8_t* text, size_t len, bool rewrite_domain, uint16_t* port16) {
    if (len && text[0] == '@') return false;                                                       // C1
    uint32_t ho, hl, po, pl;
    if (hyobfs_addr_split(text, len, &ho, &hl, &po, &pl) != HYOBFS_OK) return false;                // C2 (and the LIMIT)
    if (!rewrite_domain) {                                                                         // C3
        uint64_t hi, lo;
        if (!hyobfs::addr::parse_ip(PtrBytes{text + ho}, hl, &hi, &lo)) return false;
    }
    const uint8_t* p = text + po;                                                                  // C4
    uint32_t at = 0;
    const bool neg = pl && p[0] == '-';
    if (pl && is_sign(p[0])) at = 1;
    if (at == pl) return false;
    uint32_t nz = pl;   // the first digit that is not '0'
    for (uint32_t i = at; i < pl; ++i) {
        if (!hyobfs::addr::is_digit(p[i])) return false;
        if (nz == pl && p[i] != '0') nz = i;
    }
    uint32_t v;
    if (!atoi_port16(PtrBytes{p + nz}, pl - nz, neg, &v)) return false;
    *port16 = (uint16_t)v;                                                                         // C5
    return true;
}

}  // namespace

extern "C" {

int hyobfs_tcp_request_parse(const uint8_t* b, size_t len, uint32_t* need, uint32_t* addr_off, uint32_t* addr_len,
                             uint32_t* consumed) {
    if (!need || !addr_off || !addr_len || !consumed || (len && !b)) return HYOBFS_ERR_INVALID;
    const Framed f = parse_framed(PtrBytes{b}, len, 0);
    *need = f.need;
    *addr_off = f.text_off;
    *addr_len = f.text_len;
    *consumed = f.consumed;
    return f.status;
}

int hyobfs_tcp_response_parse(const uint8_t* b, size_t len, uint32_t* need, uint8_t* ok, uint32_t* msg_off,
                              uint32_t* msg_len, uint32_t* consumed) {
    if (!need || !ok || !msg_off || !msg_len || !consumed || (len && !b)) return HYOBFS_ERR_INVALID;
    const Framed f = parse_framed(PtrBytes{b}, len, 1);
    *need = f.need;
    *ok = f.status == HYOBFS_OK && b[0] == 0;
    *msg_off = f.text_off;
    *msg_len = f.text_len;
    *consumed = f.consumed;
    return f.status;
}

int64_t hyobfs_tcp_request_build(const uint8_t* addr, size_t addr_len, uint32_t pad_len, uint64_t seed, uint64_t item,
                                 uint8_t* out, size_t cap) {
    if ((addr_len && !addr) || (cap && !out)) return HYOBFS_ERR_INVALID;
    const uint8_t lead[2] = {varint_byte(HYOBFS_REQ_FRAME_TYPE, 2, 0), varint_byte(HYOBFS_REQ_FRAME_TYPE, 2, 1)};
    static_assert(HYOBFS_REQ_FRAME_TYPE > 63 && HYOBFS_REQ_FRAME_TYPE <= 16383, "a two-byte varint");
    return build(2, lead, addr, addr_len, pad_len, seed, item, out, cap);
}

int64_t hyobfs_tcp_response_build(int ok, const uint8_t* msg, size_t msg_len, uint32_t pad_len, uint64_t seed,
                                  uint64_t item, uint8_t* out, size_t cap) {
    if ((msg_len && !msg) || (cap && !out)) return HYOBFS_ERR_INVALID;
    const uint8_t lead[1] = {(uint8_t)(ok ? 0 : 1)};
    return build(1, lead, msg, msg_len, pad_len, seed, item, out, cap);
}

void hyobfs_req_padding_fill(uint64_t seed, uint64_t item, uint8_t* out, size_t len) {
    if (!out) return;
    const uint64_t s = pad_state(seed, item);
    for (size_t k = 0; k < len; ++k) out[k] = pad_byte(s, k);
}

int hyobfs_port_union_parse(const uint8_t* text, size_t len, hyobfs_port_range* ranges, uint32_t cap,
                            uint32_t* n_ranges) {
    if (!n_ranges || (len && !text) || (cap && !ranges)) return HYOBFS_ERR_INVALID;
    *n_ranges = 0;
    std::vector<hyobfs_port_range> u;
    if ((len == 3 && memcmp(text, "all", 3) == 0) || (len == 1 && text[0] == '*')) {
        u.push_back({0, 65535});
    } else {
        for (size_t at = 0;; ) {   // strings.Split(s, ","): the empty text is one empty part
            size_t end = at;
            while (end < len && text[end] != ',') ++end;
            const uint8_t* part = text + at;
            const size_t n = end - at;
            const uint8_t* dash = n ? (const uint8_t*)memchr(part, '-', n) : nullptr;
            uint16_t a, b;
            if (dash) {
                const size_t l = (size_t)(dash - part);
                if (memchr(dash + 1, '-', n - l - 1)) return HYOBFS_REQ_ERR_UNION;   // more than two parts
                if (!parse_u16(part, l, &a) || !parse_u16(dash + 1, n - l - 1, &b)) return HYOBFS_REQ_ERR_UNION;
                if (a > b) std::swap(a, b);
            } else {
                if (!parse_u16(part, n, &a)) return HYOBFS_REQ_ERR_UNION;
                b = a;
            }
            u.push_back({a, b});
            if (end == len) break;
            at = end + 1;
        }
    }
    std::sort(u.begin(), u.end(), [](const hyobfs_port_range& x, const hyobfs_port_range& y) {
        return x.start == y.start ? x.end < y.end : x.start < y.start;
    });
    std::vector<hyobfs_port_range> norm{u[0]};
    for (size_t i = 1; i < u.size(); ++i) {
        hyobfs_port_range& last = norm.back();
        if ((uint32_t)u[i].start <= (uint32_t)last.end + 1) {
            if (u[i].end > last.end) last.end = u[i].end;
        } else {
            norm.push_back(u[i]);
        }
    }
    *n_ranges = (uint32_t)norm.size();
    if (norm.size() > cap) return HYOBFS_REQ_ERR_CAP;
    memcpy(ranges, norm.data(), norm.size() * sizeof(hyobfs_port_range));
    return HYOBFS_OK;
}

int hyobfs_port_union_contains(const hyobfs_port_range* ranges, int64_t n_ranges, uint16_t port) {
    if (n_ranges > 0 && !ranges) return HYOBFS_ERR_INVALID;
    return contains(ranges, n_ranges, port) ? 1 : 0;
}

int hyobfs_sniff_check(const uint8_t* text, size_t len, int is_udp, int rewrite_domain, const hyobfs_port_range* tcp,
                       int64_t n_tcp, const hyobfs_port_range* udp, int64_t n_udp) {
    if ((len && !text) || (n_tcp > 0 && !tcp) || (n_udp > 0 && !udp)) return HYOBFS_ERR_INVALID;
    uint16_t port;
    if (!check_port(text, len, rewrite_domain != 0, &port)) return 0;
    return (is_udp ? contains(udp, n_udp, port) : contains(tcp, n_tcp, port)) ? 1 : 0;   // C6
}

int64_t hyobfs_request_rewrite(const uint8_t* addr, size_t addr_len, int check, const uint8_t* name, size_t name_len,
                               int32_t sniff_status, uint8_t* out, size_t cap, uint8_t* rewritten) {
    if (!rewritten || (addr_len && !addr) || (name_len && !name) || (cap && !out) || name_len > 0xFFFFFFFFull)
        return HYOBFS_ERR_INVALID;
    *rewritten = 0;
    const RewriteMode m = rewrite_mode(check != 0, sniff_status, (uint32_t)name_len);
    if (m == kLeftToHost) return HYOBFS_REQ_ERR_HOST;
    if (m == kCopy) {
        if (addr_len > cap) return -1;
        if (addr_len) memcpy(out, addr, addr_len);
        return (int64_t)addr_len;
    }
    size_t colon = addr_len;   // the last ':'
    while (colon > 0 && addr[colon - 1] != ':') --colon;
    if (colon == 0) return HYOBFS_ADDR_ERR_MISSING_PORT;
    bool br = false;
    for (size_t i = 0; i < name_len; ++i) br |= needs_brackets(name[i]);
    const size_t port_len = addr_len - colon, total = name_len + (br ? 2 : 0) + 1 + port_len;
    if (total > cap) return -1;
    size_t at = 0;
    if (br) out[at++] = '[';
    memcpy(out + at, name, name_len);
    at += name_len;
    if (br) out[at++] = ']';
    out[at++] = ':';
    if (port_len) memcpy(out + at, addr + colon, port_len);
    *rewritten = 1;
    return (int64_t)total;
}

}  // extern "C"
