// udpmsg_host.cpp -- host side of the UDP relay message (include/hyobfs_udpmsg.h):
// HeaderSize / Serialize / ParseUDPMessage (proxy.go:169-223), FragUDPMessage
// (frag.go:7-34), sendMessageAutoFrag (server/udp.go:218-235) and the Defragger
// (frag.go:40-80) as a state machine over the caller's tags.  Plain host C++; the
// device batch calls live in udpmsg.hip.
#include <cstring>
#include <new>

#include "udpmsg_rules.h"

using namespace hyobfs::udpmsg;

// Defragger (frag.go:40-45): pktID, frags (here: which slots are filled and the
// tag of each) and count.  `size` has no counterpart: no payload is touched.
struct hyobfs_udp_defragger {
    uint16_t pkt_id = 0;
    uint32_t slots = 0;   // len(d.frags)
    uint32_t count = 0;
    bool filled[HYOBFS_UDP_MAX_FRAGS] = {};
    uint64_t tags[HYOBFS_UDP_MAX_FRAGS] = {};
};

namespace {

// the header of one datagram at p: hdr_len bytes
void put_header(uint8_t* p, uint32_t session_id, uint16_t packet_id, uint8_t frag_id, uint8_t frag_count,
                const uint8_t* addr, uint32_t addr_len) {
    p[0] = (uint8_t)(session_id >> 24);
    p[1] = (uint8_t)(session_id >> 16);
    p[2] = (uint8_t)(session_id >> 8);
    p[3] = (uint8_t)session_id;
    p[4] = (uint8_t)(packet_id >> 8);
    p[5] = (uint8_t)packet_id;
    p[6] = frag_id;
    p[7] = frag_count;
    const uint32_t vl = varint_len(addr_len);
    for (uint32_t k = 0; k < vl; ++k) p[8 + k] = varint_byte(addr_len, vl, k);
    if (addr_len) memcpy(p + 8 + vl, addr, addr_len);
}

}  // namespace

extern "C" {

uint32_t hyobfs_udp_header_size(uint32_t addr_len) {
    const uint64_t h = header_size(addr_len);
    return h > UINT32_MAX ? UINT32_MAX : (uint32_t)h;   // saturates (an address within 12 bytes of 4 GiB)
}

int64_t hyobfs_udp_serialize(const hyobfs_udp_header* hdr, const uint8_t* addr, uint32_t addr_len, const uint8_t* data,
                             uint32_t data_len, uint8_t* out, size_t cap) {
    if (!hdr || (addr_len && !addr) || (data_len && !data)) return -1;
    const uint64_t h = header_size(addr_len), size = h + data_len;
    if (cap < size || !out) return -1;   // proxy.go:180-182
    put_header(out, hdr->session_id, hdr->packet_id, hdr->frag_id, hdr->frag_count, addr, addr_len);
    if (data_len) memcpy(out + h, data, data_len);
    return (int64_t)size;
}

int hyobfs_udp_parse(const uint8_t* in, size_t len, hyobfs_udp_parsed* out) {
    if (!out || (len && !in)) return HYOBFS_ERR_INVALID;
    parse(in, len, out);
    return out->status;
}

int hyobfs_udp_frag_plan(uint32_t addr_len, uint32_t data_len, uint32_t max_size, uint32_t* count,
                         uint32_t* max_payload) {
    if (!count || !max_payload) return HYOBFS_ERR_INVALID;
    return frag_plan(addr_len, data_len, max_size, count, max_payload);
}

int hyobfs_udp_send_frags(const hyobfs_udp_meta* meta, const uint8_t* addr, const uint8_t* data, uint32_t data_len,
                          uint8_t* out, size_t cap, uint32_t* dgram_len, uint32_t* count) {
    if (!meta || !count || !dgram_len || (meta->addr_len && !addr) || (data_len && !data)) return HYOBFS_ERR_INVALID;
    *count = 0;
    const SendPlan p = send_plan(meta->addr_len, data_len, meta->max_size);
    if (p.status != HYOBFS_OK) return p.status;
    if (cap < p.bytes || !out) return HYOBFS_UDP_ERR_CAP;
    const uint16_t pid = p.count == 1 ? 0 : meta->packet_id;   // udp.go:219-229
    for (uint32_t k = 0; k < p.count; ++k) {
        uint8_t* d = out + (size_t)k * p.stride;
        const uint32_t from = k * p.max_payload, take = data_len - from < p.max_payload ? data_len - from : p.max_payload;
        put_header(d, meta->session_id, pid, (uint8_t)k, (uint8_t)p.count, addr, meta->addr_len);
        if (take) memcpy(d + p.hdr, data + from, take);
        dgram_len[k] = p.hdr + take;
    }
    *count = p.count;
    return HYOBFS_OK;
}

hyobfs_udp_defragger* hyobfs_udp_defragger_new(void) { return new (std::nothrow) hyobfs_udp_defragger(); }

void hyobfs_udp_defragger_free(hyobfs_udp_defragger* d) { delete d; }

int hyobfs_udp_defragger_feed(hyobfs_udp_defragger* d, const hyobfs_udp_parsed* m, uint64_t tag, uint64_t* tags_out,
                              uint32_t* n_out) {
    if (!d || !m || !tags_out || !n_out || m->status != HYOBFS_OK) return HYOBFS_ERR_INVALID;
    *n_out = 0;
    if (m->frag_count <= 1) {   // D1, frag.go:48-50
        tags_out[0] = tag;
        *n_out = 1;
        return HYOBFS_UDP_WHOLE;
    }
    if (m->frag_id >= m->frag_count) return HYOBFS_UDP_ERR_FRAG_ID;   // D2, :51-54
    if (m->packet_id != d->pkt_id || m->frag_count != d->slots) {      // D3, :55-61
        d->pkt_id = m->packet_id;
        d->slots = m->frag_count;
        memset(d->filled, 0, sizeof d->filled);
        d->filled[m->frag_id] = true;
        d->tags[m->frag_id] = tag;
        d->count = 1;
    } else if (!d->filled[m->frag_id]) {   // D4: a filled slot is ignored, :62
        d->filled[m->frag_id] = true;
        d->tags[m->frag_id] = tag;
        if (++d->count == d->slots) {   // D5, :66-77; the state stays as it is (D6)
            memcpy(tags_out, d->tags, d->slots * sizeof(uint64_t));
            *n_out = d->slots;
            return HYOBFS_UDP_COMPLETE;
        }
    }
    return HYOBFS_UDP_PENDING;
}

}  // extern "C"
