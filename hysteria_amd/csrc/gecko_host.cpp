// gecko_host.cpp -- host side of the Gecko frame codec (include/hyobfs_gecko.h):
// encodeFrame / decodeFrame (gecko_frame.go:39-86), randomPadLen
// (gecko.go:131-138) and the reassembly table (acceptChunk and its maintenance,
// gecko.go:199-304) as a state machine over the caller's tags.  Plain host C++;
// the device batch calls live in gecko.hip and hyobfs_api.cpp.
#include <errno.h>
#include <sys/random.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/hyobfs_gecko.h"

// geckoPacketConn's reassembly state (gecko.go:69-81): reassembly, perSource, mu.
// An entry holds tags and lengths where the reference holds chunk copies.
struct hyobfs_gecko_reassembler {
    struct Entry {   // reassemblyEntry (gecko.go:62-67)
        uint64_t deadline = 0, seq = 0;   // seq: creation order, the tie rule of the header
        uint32_t total = 0, received = 0, filled = 0;   // filled: bit i = chunk i is there
        uint64_t tags[HYOBFS_GECKO_MAX_CHUNKS] = {};
        uint32_t lens[HYOBFS_GECKO_MAX_CHUNKS] = {};
    };
    using Key = std::string;   // the source's bytes, then the msg_id byte
    mutable std::mutex mu;
    std::unordered_map<Key, Entry> reassembly;
    std::unordered_map<std::string, uint32_t> per_source;
    std::map<std::pair<uint64_t, uint64_t>, Key> by_deadline;   // (deadline, seq) -> key: eviction and gc order
    std::vector<uint64_t> released;   // tags of dropped entries, not yet drained
    uint64_t next_seq = 0;

    // dropEntryLocked (gecko.go:277-286); k by value: a caller may pass by_deadline's copy, erased here.
    // Everything that can throw (the copies, room for the tags) comes before the first change.
    void drop_entry(Key k, bool release) {
        auto it = reassembly.find(k);
        if (it == reassembly.end()) return;
        const Entry& e = it->second;
        const std::string source = k.substr(0, k.size() - 1);
        if (release) {
            released.reserve(released.size() + HYOBFS_GECKO_MAX_CHUNKS);
            for (uint32_t i = 0; i < e.total; ++i)
                if (e.filled >> i & 1) released.push_back(e.tags[i]);
        }
        by_deadline.erase({e.deadline, e.seq});
        auto ps = per_source.find(source);
        if (ps != per_source.end() && --ps->second == 0) per_source.erase(ps);
        reassembly.erase(it);
    }

    // acceptChunk (gecko.go:199-249) for a FRAGMENT record decodeFrame could have produced; may throw bad_alloc,
    // leaving the table consistent
    int accept_chunk(const uint8_t* src, uint32_t source_len, const hyobfs_gecko_parsed& rec, uint64_t tag, uint64_t now_ms,
                     uint64_t* tags_out, uint32_t* n_out, uint32_t* msg_len) {
        const unsigned total = rec.idx_total & 0x0f, idx = rec.idx_total >> 4;
        const std::string source(reinterpret_cast<const char*>(src), source_len);
        const Key key = source + (char)rec.msg_id;
        std::lock_guard<std::mutex> lk(mu);
        auto it = reassembly.find(key);
        if (it == reassembly.end()) {
            auto ps = per_source.find(source);
            if (ps != per_source.end() && ps->second >= HYOBFS_GECKO_MAX_PER_SOURCE) return HYOBFS_GECKO_RX_DROPPED;   // 1
            if (reassembly.size() >= HYOBFS_GECKO_MAX_REASSEMBLY)   // 2: evictOldestLocked, the first created of equals
                drop_entry(by_deadline.begin()->second, true);
            Entry e;
            e.total = total;
            e.deadline = now_ms + HYOBFS_GECKO_REASSEMBLY_TTL_MS;   // 3
            e.seq = next_seq;
            const auto bd = by_deadline.emplace(std::make_pair(e.deadline, e.seq), key).first;
            try {
                ps = per_source.emplace(source, 0u).first;
                try {
                    it = reassembly.emplace(key, e).first;
                } catch (...) {
                    if (ps->second == 0) per_source.erase(ps);
                    throw;
                }
            } catch (...) {
                by_deadline.erase(bd);
                throw;
            }
            ++ps->second;
            ++next_seq;
        } else if (it->second.total != total) {
            return HYOBFS_GECKO_RX_DROPPED;   // 4
        }
        Entry& e = it->second;
        if (e.filled >> idx & 1) return HYOBFS_GECKO_RX_DROPPED;   // 5
        if (e.received + 1 == e.total) {   // 7: the last chunk; the entry goes first, which is all that can throw
            uint64_t sum = rec.payload_len;
            for (unsigned i = 0; i < e.total; ++i) {
                tags_out[i] = i == idx ? tag : e.tags[i];
                sum += i == idx ? 0 : e.lens[i];
            }
            const uint32_t n = e.total;
            drop_entry(key, false);
            *n_out = n;
            *msg_len = sum > UINT32_MAX ? UINT32_MAX : (uint32_t)sum;
            return HYOBFS_GECKO_RX_COMPLETE;
        }
        e.filled |= 1u << idx;   // 6
        e.tags[idx] = tag;
        e.lens[idx] = rec.payload_len;
        ++e.received;
        return HYOBFS_GECKO_RX_PENDING;   // 8
    }
};

namespace {

bool fill_random(uint8_t* p, size_t n) {   // crypto/rand.Read
    while (n) {
        const ssize_t r = getrandom(p, n, 0);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}

bool chunks_ok(unsigned total, unsigned idx) {
    return total >= HYOBFS_GECKO_MIN_CHUNKS && total <= HYOBFS_GECKO_MAX_CHUNKS && idx < total;
}

}  // namespace

extern "C" {

int hyobfs_gecko_random_pad_key(uint8_t key[32], uint8_t nonce[12]) {   // crypto/rand, gecko_frame.go:55
    if (!key || !nonce) return HYOBFS_ERR_INVALID;
    return fill_random(key, 32) && fill_random(nonce, 12) ? HYOBFS_OK : HYOBFS_ERR_IO;
}

int64_t hyobfs_gecko_encode_frame(const hyobfs_gecko_header* h, const uint8_t* payload, size_t len, uint8_t* out,
                                  size_t cap) {
    if (!h || !chunks_ok(h->total_chunks, h->chunk_idx)) return HYOBFS_GECKO_ERR_INVALID;
    const size_t needed = HYOBFS_GECKO_HEADER_LEN + (size_t)h->pad_len + len;
    if (!out || cap < needed) return HYOBFS_GECKO_ERR_TRUNCATED;
    out[0] = HYOBFS_GECKO_FLAG_FRAGMENT;
    out[1] = h->msg_id;
    out[2] = (uint8_t)(h->chunk_idx << 4 | (h->total_chunks & 0x0f));
    out[3] = (uint8_t)(h->pad_len >> 8);   // big-endian
    out[4] = (uint8_t)h->pad_len;
    if (!fill_random(out + HYOBFS_GECKO_HEADER_LEN, h->pad_len)) return HYOBFS_ERR_IO;
    if (len) std::memmove(out + HYOBFS_GECKO_HEADER_LEN + h->pad_len, payload, len);
    return (int64_t)needed;
}

int hyobfs_gecko_decode_frame(const uint8_t* in, size_t len, hyobfs_gecko_header* h, size_t* payload_off) {
    if (len < HYOBFS_GECKO_HEADER_LEN || !in) return HYOBFS_GECKO_ERR_TRUNCATED;
    if (!(in[0] & HYOBFS_GECKO_FLAG_FRAGMENT)) return HYOBFS_GECKO_ERR_INVALID;
    hyobfs_gecko_header r{};
    r.msg_id = in[1];
    r.chunk_idx = in[2] >> 4;
    r.total_chunks = in[2] & 0x0f;
    r.pad_len = (uint16_t)((in[3] << 8) | in[4]);
    if (!chunks_ok(r.total_chunks, r.chunk_idx)) return HYOBFS_GECKO_ERR_INVALID;
    if (HYOBFS_GECKO_HEADER_LEN + (size_t)r.pad_len > len) return HYOBFS_GECKO_ERR_TRUNCATED;
    if (h) *h = r;
    if (payload_off) *payload_off = HYOBFS_GECKO_HEADER_LEN + r.pad_len;
    return HYOBFS_OK;
}

uint32_t hyobfs_gecko_pad_len(int min_pkt, int max_pkt, uint32_t chunk_len, uint32_t rnd) {
    const int64_t base = HYOBFS_SALT_LEN + HYOBFS_GECKO_HEADER_LEN + (int64_t)chunk_len;
    const int64_t lo = std::max<int64_t>(min_pkt, base);
    if (lo > max_pkt) return 0;
    const int64_t span = (int64_t)max_pkt - lo + 1;   // randIntn(span)
    const int64_t r = span <= 1 ? 0 : (int64_t)(rnd % (uint32_t)span);
    return (uint32_t)(lo - base + r);
}

hyobfs_gecko_reassembler* hyobfs_gecko_reassembler_new(void) { return new (std::nothrow) hyobfs_gecko_reassembler(); }

void hyobfs_gecko_reassembler_free(hyobfs_gecko_reassembler* r) { delete r; }

int hyobfs_gecko_reassembler_feed(hyobfs_gecko_reassembler* r, const uint8_t* source, uint32_t source_len,
                                  const hyobfs_gecko_parsed* rec, uint64_t tag, uint64_t now_ms, uint64_t tags_out[8],
                                  uint32_t* n_out, uint32_t* msg_len) {
    if (!r || !rec || !tags_out || !n_out || !msg_len || (source_len && !source)) return HYOBFS_ERR_INVALID;
    *n_out = 0;
    *msg_len = 0;
    if (rec->status == HYOBFS_GECKO_PASS) {   // gecko.go:183-185
        tags_out[0] = tag;
        *n_out = 1;
        *msg_len = rec->payload_len;
        return HYOBFS_GECKO_RX_PASS;
    }
    if (rec->status != HYOBFS_GECKO_FRAGMENT || !chunks_ok(rec->idx_total & 0x0f, rec->idx_total >> 4))
        return HYOBFS_GECKO_RX_DROPPED;   // :178-190
    try {
        return r->accept_chunk(source, source_len, *rec, tag, now_ms, tags_out, n_out, msg_len);
    } catch (const std::bad_alloc&) {   // the ABI is plain C
        return HYOBFS_ERR_NOMEM;
    }
}

void hyobfs_gecko_reassembler_gc(hyobfs_gecko_reassembler* r, uint64_t now_ms) {   // gcExpired (gecko.go:266-274)
    if (!r) return;
    std::lock_guard<std::mutex> lk(r->mu);
    try {
        while (!r->by_deadline.empty() && now_ms > r->by_deadline.begin()->first.first)
            r->drop_entry(r->by_deadline.begin()->second, true);
    } catch (const std::bad_alloc&) {   // out of memory: the entries not yet dropped stay for the next call
    }
}

uint64_t hyobfs_gecko_reassembler_pending(const hyobfs_gecko_reassembler* r) {
    if (!r) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    return r->reassembly.size();
}

uint64_t hyobfs_gecko_reassembler_released(hyobfs_gecko_reassembler* r, uint64_t* tags, uint64_t cap) {
    if (!r) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    if (!tags || cap == 0) return r->released.size();
    const uint64_t k = std::min<uint64_t>(cap, r->released.size());
    std::copy(r->released.begin(), r->released.begin() + (ptrdiff_t)k, tags);
    r->released.erase(r->released.begin(), r->released.begin() + (ptrdiff_t)k);
    return k;
}

}  // extern "C"
