// addr_host.cpp -- host side of the request address (include/hyobfs_addr.h):
// net.SplitHostPort, parsePortUint16 (extras/outbounds/interface.go:71-77),
// tryParseIP (utils.go:29-40) and AddrEx.String() (interface.go:49-51) for one
// address.  Plain host C++; the device batch calls live in addr.hip.
#include <cstring>

#include "addr_rules.h"

using namespace hyobfs::addr;

namespace {

void put_be64(uint8_t* p, uint64_t v) {
    for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (56 - 8 * k));
}
uint64_t get_be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v = v << 8 | p[k];
    return v;
}

// rule H (and the LIMIT) over text[0, len): one pass collects what SplitHostPort looks at
Split split(const uint8_t* text, size_t len) {
    if (len > HYOBFS_UDP_MAX_ADDR) return split_fail(HYOBFS_ADDR_ERR_TOO_LONG);
    SplitFacts f{(uint32_t)len, kNone, kNone, kNone, kNone, false, false, false};
    for (uint32_t i = 0; i < (uint32_t)len; ++i) {
        const uint8_t c = text[i];
        if (c == ':') {
            if (f.first_colon == kNone) f.first_colon = i;
            f.last_colon = i;
        } else if (c == ']') {
            if (f.first_rb == kNone) f.first_rb = i;
            f.last_rb = i;
        } else if (c == '[') {
            if (i == 0) f.lb0 = true;
            else f.lb_later = true;
        }
    }
    f.colon_after_rb = f.first_rb != kNone && f.first_rb + 1 < f.len && text[f.first_rb + 1] == ':';
    return split_decide(f);
}

// rule P over p[0, n)
bool parse_port(const uint8_t* p, size_t n, uint32_t* v) {
    *v = 0;
    if (n == 0) return false;
    size_t nz = n;   // the first byte that is not '0'
    for (size_t i = 0; i < n; ++i) {
        if (!is_digit(p[i])) return false;
        if (nz == n && p[i] != '0') nz = i;
    }
    return port_value(PtrBytes{p + nz}, n - nz > 6 ? 6u : (uint32_t)(n - nz), v);
}

}  // namespace

extern "C" {

int hyobfs_addr_split(const uint8_t* text, size_t len, uint32_t* host_off, uint32_t* host_len, uint32_t* port_off,
                      uint32_t* port_len) {
    if (!host_off || !host_len || !port_off || !port_len || (len && !text)) return HYOBFS_ERR_INVALID;
    const Split s = split(text, len);
    *host_off = s.host_off;
    *host_len = s.host_len;
    *port_off = s.port_off;
    *port_len = s.port_len;
    return s.status;
}

int hyobfs_addr_parse_port(const uint8_t* text, size_t len, uint16_t* port) {
    if (!port || (len && !text)) return HYOBFS_ERR_INVALID;
    uint32_t v;
    const bool ok = parse_port(text, len, &v);
    *port = (uint16_t)v;
    return ok ? HYOBFS_OK : HYOBFS_ADDR_ERR_PORT;
}

int hyobfs_addr_parse_ip(const uint8_t* text, size_t len, uint8_t* ip16) {
    if (!ip16 || (len && !text)) return HYOBFS_ERR_INVALID;
    uint64_t hi = 0, lo = 0;
    const bool ok = len <= HYOBFS_ADDR_LITERAL_MAX && parse_ip(PtrBytes{text}, (uint32_t)len, &hi, &lo);
    put_be64(ip16, hi);
    put_be64(ip16 + 8, lo);
    return ok ? 1 : 0;
}

int hyobfs_addr_parse(const uint8_t* text, size_t len, uint32_t* name_off, uint32_t* name_len, uint8_t* ipv4,
                      uint8_t* ipv6, uint8_t* ip_flags, uint16_t* port) {
    if (!name_off || !name_len || !ipv4 || !ipv6 || !ip_flags || !port || (len && !text)) return HYOBFS_ERR_INVALID;
    *name_off = *name_len = 0;
    memset(ipv4, 0, 4);
    memset(ipv6, 0, 16);
    *ip_flags = 0;
    *port = 0;
    const Split s = split(text, len);
    if (s.status != HYOBFS_OK) return s.status;
    uint32_t v;
    if (!parse_port(text + s.port_off, s.port_len, &v)) return HYOBFS_ADDR_ERR_PORT;
    *name_off = s.host_off;
    *name_len = s.host_len;
    *port = (uint16_t)v;
    uint64_t hi, lo;
    if (parse_ip(PtrBytes{text + s.host_off}, s.host_len, &hi, &lo)) {   // rule T
        if (is_v4_mapped(hi, lo)) {
            *ip_flags = HYOBFS_ADDR_HAS_IPV4;
            for (int k = 0; k < 4; ++k) ipv4[k] = (uint8_t)(lo >> (24 - 8 * k));
        } else {
            *ip_flags = HYOBFS_ADDR_HAS_IPV6;
            put_be64(ipv6, hi);
            put_be64(ipv6 + 8, lo);
        }
    }
    return HYOBFS_OK;
}

int hyobfs_addr_format(const uint8_t* ip, uint32_t family, uint16_t port, uint8_t* out, size_t cap) {
    if (!ip || (cap && !out)) return HYOBFS_ERR_INVALID;
    if (family != 4 && family != 16) return HYOBFS_ADDR_ERR_FAMILY;
    uint8_t text[HYOBFS_ADDR_FORMAT_MAX + 1];
    const uint64_t hi = family == 4 ? (uint64_t)ip[0] << 56 | (uint64_t)ip[1] << 48 | (uint64_t)ip[2] << 40 | (uint64_t)ip[3] << 32
                                    : get_be64(ip);
    const int n = format(hi, family == 4 ? 0 : get_be64(ip + 8), family, port, text);
    if (n < 0) return n;
    if ((size_t)n > cap) return -1;
    memcpy(out, text, (size_t)n);
    return n;
}

}  // extern "C"
