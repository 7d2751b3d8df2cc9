/*
 * hyobfs_gecko.h -- Gecko framing (extras/obfs/gecko_frame.go, gecko.go) on
 * top of the Salamander context of hyobfs.h.
 *
 * Gecko fragments QUIC long-header packets into 2..8 chunks, each sent as its
 * own Salamander datagram
 *     salt(8) || ( 0x80 | msgID | chunkIdx<<4|total | padLen(BE16) | pad | chunk ) ^ key
 * and padded so the datagram lands in [min_pkt, max_pkt]; short-header packets
 * pass through as plain Salamander datagrams.  The per-byte work runs on the
 * GPU in both directions; the random choices (chunk counts, pad lengths,
 * msgIDs) and the reassembly table stay on the host, as in the reference.
 *
 *   reference (Go)                                   here
 *   ------------------------------------------------ ------------------------------------------------
 *   encodeFrame (gecko_frame.go:39-61)               hyobfs_gecko_encode_frame
 *   decodeFrame (gecko_frame.go:65-86)               hyobfs_gecko_decode_frame
 *   randomPadLen (gecko.go:131-138)                  hyobfs_gecko_pad_len
 *   writeFragmented + Obfuscate (gecko.go:112-129)   hyobfs_gecko_encode_batch (device: header, padding,
 *                                                    chunk and the XOR in one pass)
 *   ReadFrom's classification (gecko.go:178-190)     hyobfs_gecko_parse_batch (device, deobfuscated input)
 *   Deobfuscate's key + that classification          hyobfs_gecko_peek_batch (device, wire input: reads the
 *   (salamander.go:74-91, gecko.go:178-190)          salt and at most five bytes of each datagram)
 *   acceptChunk (gecko.go:199-249), the map and      hyobfs_gecko_reassembler_feed (host, over the caller's
 *   its two caps                                     tags: no payload byte is touched)
 *   gcExpired (gecko.go:266-274)                     hyobfs_gecko_reassembler_gc
 *   evictOldestLocked (gecko.go:290-304)             inside _feed (rule 2 there; the tie rule is stated)
 *   len(g.reassembly)                                hyobfs_gecko_reassembler_pending
 *   (the chunk copies the garbage collector frees)   hyobfs_gecko_reassembler_released
 *   acceptChunk's copies + Deobfuscate's XOR         hyobfs_gecko_open_batch (device: only payload bytes
 *   (gecko.go:230-246, salamander.go:82-84)          are read, XORed and written, once)
 *
 * Plain C ABI: pointers, sizes, integer status codes.
 */
#ifndef HYOBFS_GECKO_H
#define HYOBFS_GECKO_H

#include <stddef.h>
#include <stdint.h>

#include "hyobfs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gecko_frame.go:9-15, gecko.go:17-26 */
#define HYOBFS_GECKO_FLAG_FRAGMENT 0x80
#define HYOBFS_GECKO_HEADER_LEN 5
#define HYOBFS_GECKO_MIN_CHUNKS 2
#define HYOBFS_GECKO_MAX_CHUNKS 8
#define HYOBFS_GECKO_BUFFER_SIZE 2048
#define HYOBFS_GECKO_DEFAULT_MIN_PACKET 512
#define HYOBFS_GECKO_DEFAULT_MAX_PACKET 1200
#define HYOBFS_GECKO_REASSEMBLY_TTL_MS 8000
#define HYOBFS_GECKO_MAX_REASSEMBLY 4096
#define HYOBFS_GECKO_MAX_PER_SOURCE 8

/* frame status codes: errFrameTruncated / errFrameInvalid (gecko_frame.go:18-21) */
#define HYOBFS_GECKO_ERR_TRUNCATED (-20)
#define HYOBFS_GECKO_ERR_INVALID (-21)
/* per-datagram parse results (hyobfs_gecko_parsed.status) */
#define HYOBFS_GECKO_PASS 0        /* top bit clear: short header or garbage, passed through (gecko.go:183-185) */
#define HYOBFS_GECKO_FRAGMENT 1    /* a valid fragment frame */
#define HYOBFS_GECKO_EMPTY (-22)   /* zero-length datagram: skipped by ReadFrom (gecko.go:178-180) */
/* per-message results of hyobfs_gecko_open_batch (status[j]) */
#define HYOBFS_GECKO_ERR_CAP (-23)   /* the message is longer than out_cap[j] */
#define HYOBFS_GECKO_ERR_PLAN (-24)  /* a chunk list that cannot be opened */
/* results of hyobfs_gecko_reassembler_feed */
#define HYOBFS_GECKO_RX_PENDING 0    /* stored; the message is not complete yet */
#define HYOBFS_GECKO_RX_PASS 1       /* not a fragment: the datagram is the message */
#define HYOBFS_GECKO_RX_COMPLETE 2   /* the last missing chunk: tags_out lists the message */
#define HYOBFS_GECKO_RX_DROPPED 3    /* dropped silently, as the reference does */

/* frameHeader (gecko_frame.go:30-35) */
typedef struct hyobfs_gecko_header {
    uint16_t pad_len;
    uint8_t msg_id;
    uint8_t chunk_idx;     /* < total_chunks */
    uint8_t total_chunks;  /* [2, 8] */
    uint8_t reserved_[3];
} hyobfs_gecko_header;

/*
 * encodeFrame (gecko_frame.go:39-61), host memory.  Writes header, pad_len
 * random bytes (getrandom, like crypto/rand) and the payload into out.
 * Returns the frame length, HYOBFS_GECKO_ERR_INVALID (chunk count or index
 * out of range) or HYOBFS_GECKO_ERR_TRUNCATED (cap too small).
 */
int64_t hyobfs_gecko_encode_frame(const hyobfs_gecko_header* h, const uint8_t* payload, size_t len,
                                  uint8_t* out, size_t cap);
/*
 * decodeFrame (gecko_frame.go:65-86), host memory.  On success fills *h and
 * *payload_off (the payload is in[*payload_off, len)) and returns HYOBFS_OK;
 * otherwise HYOBFS_GECKO_ERR_TRUNCATED or HYOBFS_GECKO_ERR_INVALID, checked in
 * the reference's order.
 */
int hyobfs_gecko_decode_frame(const uint8_t* in, size_t len, hyobfs_gecko_header* h, size_t* payload_off);
/*
 * randomPadLen (gecko.go:131-138) with the randomness passed in: rnd is a
 * uniform 32-bit value (randIntn's BigEndian.Uint32 of 4 random bytes,
 * gecko.go:145-153).  Padding puts salt + header + pad + chunk in
 * [min_pkt, max_pkt]; 0 when the chunk alone exceeds max_pkt.
 */
uint32_t hyobfs_gecko_pad_len(int min_pkt, int max_pkt, uint32_t chunk_len, uint32_t rnd);

/* ------------------------------------------------ device batch: send side */
/* One wire datagram (frame) of a fragmented message, planned on the host
 * (writeFragmented, gecko.go:107-129): the chunk is msg[chunk_off, +chunk_len). */
typedef struct hyobfs_gecko_frame {
    uint64_t chunk_off;
    uint32_t chunk_len;
    uint16_t pad_len;
    uint8_t msg_id;
    uint8_t idx_total;     /* chunkIdx << 4 | totalChunks, the wire's byte 2 */
} hyobfs_gecko_frame;

typedef struct hyobfs_gecko_batch {
    uint64_t n;                          /* frames */
    const uint8_t* msg;                  /* message bytes (device) */
    const hyobfs_gecko_frame* frames;    /* n frames (device) */
    const uint64_t* salts;               /* n Salamander salts (device), as hyobfs_batch.salts */
    /* Padding (the reference fills it from crypto/rand, gecko_frame.go:55): a keyed
       keystream, ChaCha with 8 rounds (the RFC 8439 block: constants, pad_key as
       8 little-endian words, a 32-bit block counter, pad_nonce as 3 words), each
       64-byte block's bytes in column order (bytes 16c..16c+15 = state words c,
       c+4, c+8, c+12 after the final addition).  Pad byte j of frame i is
       keystream byte out_off[i] + 13 + j: its offset in `out`, so every pad byte
       of a batch takes a different keystream byte.  Block b (64-bit) uses
       counter = b mod 2^32 and nonce word 0 XOR (b >> 32): no block repeats at
       any offset.  Draw a fresh key per batch (hyobfs_gecko_random_pad_key,
       getrandom); an explicit key makes the output reproducible (tests,
       oracle/gecko_ref.py).  An all-zero pad_key is rejected
       (HYOBFS_ERR_INVALID): it is what a caller that forgot the key passes. */
    uint8_t pad_key[32];
    uint8_t pad_nonce[12];
    uint32_t reserved_;
    uint8_t* out;                        /* device */
    const uint64_t* out_off;             /* frame i's wire datagram at out + out_off[i] (device);
                                            its length is 8 + 5 + pad_len + chunk_len */
    void* workspace;                     /* ignored (ABI 3: the encode kernel needs no scratch) */
    uint64_t workspace_bytes;            /* ignored */
    uint64_t out_cap;                    /* ignored (ABI 2 used it for the wire-tile kernel, since removed) */
} hyobfs_gecko_batch;

/* 0: kept for callers of ABI 1 (the wave-group kernel needs no workspace). */
uint64_t hyobfs_gecko_workspace_size(uint64_t n);
/* A fresh 256-bit pad key and 96-bit nonce from the OS (getrandom, the source of
   crypto/rand).  Returns HYOBFS_OK or HYOBFS_ERR_IO. */
int hyobfs_gecko_random_pad_key(uint8_t key[32], uint8_t nonce[12]);
/*
 * Encode and obfuscate every frame in one pass on the context's device:
 * out = salt || (header || pad || chunk) ^ BLAKE2b-256(PSK || salt)[i % 32]
 * (encodeFrame + Salamander Obfuscate, gecko.go:120-128 -> salamander.go:59-72).
 * Asynchronous on `stream` (NULL = null stream).  A frame the reference could
 * not have produced (total chunks outside [2, 8], chunk index >= total, or a
 * datagram longer than HYOBFS_GECKO_BUFFER_SIZE) is skipped on the device: its
 * output bytes are left untouched.  HYOBFS_ERR_INVALID for a missing pointer
 * or an all-zero pad_key.
 */
int hyobfs_gecko_encode_batch(hyobfs_salamander* ctx, const hyobfs_gecko_batch* b, void* stream);

/* --------------------------------------------- device batch: receive side */
typedef struct hyobfs_gecko_parsed {
    int32_t status;        /* HYOBFS_GECKO_PASS / _FRAGMENT / _EMPTY / _ERR_TRUNCATED / _ERR_INVALID */
    uint16_t pad_len;
    uint8_t msg_id;
    uint8_t idx_total;     /* chunkIdx << 4 | totalChunks */
    uint32_t payload_off;  /* payload = datagram[payload_off, payload_off + payload_len) */
    uint32_t payload_len;
} hyobfs_gecko_parsed;

/*
 * Classify and parse n deobfuscated datagrams (ReadFrom, gecko.go:170-193 ->
 * decodeFrame): datagram i is in[in_off[i], +in_len[i]) (device pointers, as
 * produced by hyobfs_salamander_deobfuscate_batch; in_len[i] == 0 marks a
 * dropped one).  One thread per datagram on the current device.
 */
int hyobfs_gecko_parse_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint64_t n,
                             hyobfs_gecko_parsed* out, void* stream);

/*
 * The receive side without the padding.  Three steps:
 *
 *   hyobfs_gecko_peek_batch       device: key and 16-byte record of every wire datagram
 *   hyobfs_gecko_reassembler_*    host: which datagrams form which message (indices only)
 *   hyobfs_gecko_open_batch       device: the payloads of every ready message, deobfuscated
 *                                 and concatenated
 *
 * A fragment datagram in the default [512, 1200] band is mostly padding, which the
 * receiver never needs: peek reads 13 bytes of it, open reads its payload only.
 *
 * peek, for each still obfuscated wire datagram wire[wire_off[i], +wire_len[i])
 * (device pointers):
 *   wire_len[i] <= 8   parsed[i] = {HYOBFS_GECKO_EMPTY, 0...}; keys[32 i, +32) is not
 *                      written (Deobfuscate returns 0, salamander.go:75-77; ReadFrom
 *                      skips it, gecko.go:178-180)
 *   otherwise          keys[32 i, +32) = BLAKE2b-256(PSK || wire[0, 8)); parsed[i] is the
 *                      record hyobfs_gecko_parse_batch writes for the deobfuscated
 *                      datagram of wire_len[i] - 8 bytes: the same checks in the same
 *                      order, payload_off / payload_len relative to that plaintext
 * It reads the salt and at most the five bytes behind it, and never a byte at or past
 * wire_off[i] + wire_len[i]; it writes parsed[0, n) and the stated key ranges only.
 * One lane per datagram; asynchronous on `stream`.  n == 0 returns HYOBFS_OK before
 * any pointer is looked at; a null pointer returns HYOBFS_ERR_INVALID.
 */
int hyobfs_gecko_peek_batch(hyobfs_salamander* ctx, const uint8_t* wire, const uint64_t* wire_off,
                            const uint32_t* wire_len, uint64_t n, hyobfs_gecko_parsed* parsed, uint8_t* keys,
                            void* stream);

/*
 * acceptChunk (gecko.go:199-249) and its maintenance (gecko.go:266-304) as a state
 * machine over the caller's 64-bit tags (a datagram's slot, say); it never sees a
 * payload byte.  `source` is opaque bytes of any length and stands for the
 * reference's addr.String(); time is the caller's millisecond clock, passed in.
 * One mutex: calls on one reassembler may come from several threads.
 *
 * feed, by rec->status:
 *   PASS       HYOBFS_GECKO_RX_PASS, tags_out[0] = tag, *n_out = 1, *msg_len =
 *              payload_len; the state is untouched (gecko.go:183-185)
 *   EMPTY,     HYOBFS_GECKO_RX_DROPPED, *n_out = 0 ("malformed frame; drop silently",
 *   ERR_*      gecko.go:187-190); so is a FRAGMENT record decodeFrame could not have
 *              produced (total outside [2, 8] or index >= total), before any state
 *   FRAGMENT   acceptChunk's rules in its order, key = (source, msg_id):
 *     1. a new key while its source has HYOBFS_GECKO_MAX_PER_SOURCE entries: DROPPED
 *     2. a new key while HYOBFS_GECKO_MAX_REASSEMBLY entries exist: the entry with the
 *        earliest deadline is evicted first
 *     3. the new entry's deadline is now_ms + HYOBFS_GECKO_REASSEMBLY_TTL_MS, set at
 *        creation and never refreshed
 *     4. an existing entry with another total: DROPPED
 *     5. a filled index: DROPPED (the first copy wins)
 *     6. otherwise the chunk's tag and payload_len are stored
 *     7. the last chunk: HYOBFS_GECKO_RX_COMPLETE, tags_out[0, total) the tags in chunk
 *        order, *n_out = total, *msg_len = the sum of the payload lengths (saturating at
 *        UINT32_MAX); the entry is deleted and its source's count decremented, so a
 *        later chunk with the same msg_id starts a new entry
 *     8. otherwise HYOBFS_GECKO_RX_PENDING, *n_out = 0
 * HYOBFS_ERR_INVALID for a null argument (source may be null when source_len is 0);
 * HYOBFS_ERR_NOMEM when the table cannot grow (the chunk is not stored, the table stays as it was,
 * but for an eviction already made).
 *
 * Stated divergence: evictOldestLocked walks a Go map, so which of several entries
 * with the same earliest deadline it drops is unspecified in the reference.  Here the
 * one created first goes.  gc likewise drops in (deadline, creation) order, which only
 * shows in the order of `released`.
 */
typedef struct hyobfs_gecko_reassembler hyobfs_gecko_reassembler;
hyobfs_gecko_reassembler* hyobfs_gecko_reassembler_new(void);
void hyobfs_gecko_reassembler_free(hyobfs_gecko_reassembler* r);
int hyobfs_gecko_reassembler_feed(hyobfs_gecko_reassembler* r, const uint8_t* source, uint32_t source_len,
                                  const hyobfs_gecko_parsed* rec, uint64_t tag, uint64_t now_ms, uint64_t tags_out[8],
                                  uint32_t* n_out, uint32_t* msg_len);
/* gcExpired: drops every entry with now_ms > deadline (strict, as now.After).  Out of memory it stops
   early; the next call goes on. */
void hyobfs_gecko_reassembler_gc(hyobfs_gecko_reassembler* r, uint64_t now_ms);
/* len(g.reassembly) */
uint64_t hyobfs_gecko_reassembler_pending(const hyobfs_gecko_reassembler* r);
/*
 * The tags of chunks whose entries gc or an eviction dropped since they were last
 * drained, oldest first: the caller frees what they stand for.  Copies at most `cap`
 * of them to `tags`, forgets those and returns their number; with tags null or cap 0 it
 * returns how many wait.  Tags handed out by a COMPLETE never appear here.
 */
uint64_t hyobfs_gecko_reassembler_released(hyobfs_gecko_reassembler* r, uint64_t* tags, uint64_t cap);

/*
 * Open m messages.  wire, wire_off, wire_len, parsed and keys are a table of n
 * datagram slots as hyobfs_gecko_peek_batch left them (device pointers); the table may
 * span many received batches, which is how chunks that arrived in different batches
 * meet.  Message j is the concatenation, in list order, of the opened payloads of the
 * slots chunk_idx[msg_first[j] .. msg_first[j + 1]); for slot c and payload byte t
 *     out = wire[wire_off[c] + 8 + payload_off + t] ^ keys[32 c + (payload_off + t) % 32]
 * (the key phase is the plaintext index, salamander.go:82-84).  A PASS record has
 * payload_off 0 and payload_len wire_len - 8, so a list of one PASS slot yields the
 * whole deobfuscated datagram.  out_len[j] = the sum of the payload lengths (taken in
 * 64 bits), the bytes at out + out_off[j].  status[j]:
 *   HYOBFS_OK
 *   HYOBFS_GECKO_ERR_CAP    the sum exceeds out_cap[j]
 *   HYOBFS_GECKO_ERR_PLAN   an empty list, more than HYOBFS_GECKO_MAX_CHUNKS entries, an
 *                           index >= n, a slot whose status is neither FRAGMENT nor PASS,
 *                           a PASS slot in a list longer than one, or a slot with
 *                           payload_off + payload_len != wire_len - 8
 * Both errors write nothing of the message and set out_len[j] = 0.  A list may name a
 * slot twice; an empty payload is legal (a 1-byte message split in two has one).
 * No byte of a datagram's salt, header or padding is read and no load leaves
 * wire[wire_off[c], +wire_len[c]); exactly out[out_off[j], +out_len[j]), out_len[0, m)
 * and status[0, m) are written.  Runs on the current device, asynchronous on `stream`.
 * m == 0 returns HYOBFS_OK before any pointer is looked at; a null pointer returns
 * HYOBFS_ERR_INVALID.
 */
int hyobfs_gecko_open_batch(const uint8_t* wire, const uint64_t* wire_off, const uint32_t* wire_len,
                            const hyobfs_gecko_parsed* parsed, const uint8_t* keys, uint64_t n,
                            const uint32_t* chunk_idx, const uint64_t* msg_first, uint64_t m, uint8_t* out,
                            const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYOBFS_GECKO_H */
