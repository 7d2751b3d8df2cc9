// udpmsg_rules.h -- the arithmetic of include/hyobfs_udpmsg.h's rules S, P, F
// and A, shared by the scalar host functions (udpmsg_host.cpp, plain C++) and
// the device kernels (udpmsg.hip, which defines HY_UDP_FN as a host/device
// qualifier before including this).  Not installed.
#pragma once
#include <stdint.h>

#include "../../include/hyobfs_udpmsg.h"

#ifndef HY_UDP_FN
#define HY_UDP_FN inline
#endif

namespace hyobfs {
namespace udpmsg {

// quicvarint.Len / varintPut (proxy.go:227-256): the minimal form
HY_UDP_FN uint32_t varint_len(uint64_t v) { return v <= 63 ? 1u : v <= 16383 ? 2u : v <= 1073741823ull ? 4u : 8u; }
HY_UDP_FN uint8_t varint_byte(uint64_t v, uint32_t vl, uint32_t k) {   // byte k of the vl written
    const uint8_t b = (uint8_t)(v >> (8 * (vl - 1 - k)));
    return k ? b : (uint8_t)(b | (vl == 1 ? 0x00 : vl == 2 ? 0x40 : vl == 4 ? 0x80 : 0xC0));
}

HY_UDP_FN uint64_t header_size(uint64_t addr_len) { return 8 + varint_len(addr_len) + addr_len; }   // proxy.go:169-172

// ParseUDPMessage (proxy.go:193-223), rule P
HY_UDP_FN void parse(const uint8_t* d, uint64_t len, hyobfs_udp_parsed* r) {
    *r = hyobfs_udp_parsed{};
    if (len < 9) {   // P1, and P2's first byte
        r->status = HYOBFS_UDP_ERR_TRUNCATED;
        return;
    }
    const uint32_t vl = 1u << (d[8] >> 6);
    if (len < 8 + vl) {   // P2
        r->status = HYOBFS_UDP_ERR_TRUNCATED;
        return;
    }
    uint64_t v = d[8] & 0x3f;
    for (uint32_t k = 1; k < vl; ++k) v = (v << 8) | d[8 + k];
    if (v == 0 || v > HYOBFS_UDP_MAX_ADDR) {   // P3
        r->status = HYOBFS_UDP_ERR_ADDR_LEN;
        return;
    }
    const uint64_t rest = len - 8 - vl;
    if (rest <= v) {   // P4
        r->status = HYOBFS_UDP_ERR_MSG_LEN;
        return;
    }
    r->status = HYOBFS_OK;
    r->session_id = (uint32_t)d[0] << 24 | (uint32_t)d[1] << 16 | (uint32_t)d[2] << 8 | d[3];
    r->packet_id = (uint16_t)(d[4] << 8 | d[5]);
    r->frag_id = d[6];
    r->frag_count = d[7];
    r->addr_off = 8 + vl;
    r->addr_len = (uint32_t)v;
    r->data_off = 8 + vl + (uint32_t)v;
    r->data_len = (uint32_t)(rest - v);
}

// FragUDPMessage (frag.go:7-34), rule F
HY_UDP_FN int frag_plan(uint64_t addr_len, uint64_t data_len, uint64_t max_size, uint32_t* count, uint32_t* max_payload) {
    const uint64_t h = header_size(addr_len);
    if (h + data_len <= max_size) {   // frag.go:8
        *count = 1;
        *max_payload = (uint32_t)data_len;
        return HYOBFS_OK;
    }
    *count = 0;
    *max_payload = 0;
    if (max_size <= h) return HYOBFS_UDP_NO_ROOM;   // :13
    const uint64_t mp = max_size - h;
    const uint64_t c = (data_len + mp - 1) / mp;   // :18, before the reference narrows it to uint8
    if (c > HYOBFS_UDP_MAX_FRAGS) return HYOBFS_UDP_ERR_FRAG_COUNT;
    *count = (uint32_t)c;
    *max_payload = (uint32_t)mp;
    return HYOBFS_OK;
}

// What rule A sends for one message.  Fragment k is the bytes [k * stride,
// min((k + 1) * stride, bytes)) of the message's output: hdr header bytes, then
// its data slice.
struct SendPlan {
    int32_t status;
    uint32_t count;         // datagrams (0 when status is not OK)
    uint32_t hdr;           // HeaderSize
    uint32_t max_payload;
    uint32_t stride;        // hdr + max_payload
    uint32_t bytes;         // count * hdr + data_len
};

HY_UDP_FN SendPlan send_plan(uint32_t addr_len, uint32_t data_len, uint32_t max_size) {
    SendPlan p{};
    const uint64_t h = header_size(addr_len);
    if (h + data_len > HYOBFS_UDP_MAX_SIZE) {   // A1: Serialize into msgBuf returns -1 (server.go:387-402)
        p.status = HYOBFS_UDP_TOO_LARGE;
        return p;
    }
    p.status = frag_plan(addr_len, data_len, max_size, &p.count, &p.max_payload);
    if (p.status != HYOBFS_OK) return p;
    p.hdr = (uint32_t)h;   // <= 4096 here
    p.stride = p.hdr + p.max_payload;
    p.bytes = p.count * p.hdr + data_len;
    return p;
}

}  // namespace udpmsg
}  // namespace hyobfs
