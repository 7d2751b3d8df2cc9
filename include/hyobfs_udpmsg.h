/*
 * hyobfs_udpmsg.h -- Hysteria's UDP relay message (apernet/hysteria
 * core/internal/protocol/proxy.go:151-256) and its fragmentation
 * (core/internal/frag/frag.go): the layer between a QUIC datagram and the
 * request hook.  Scalar host functions, and three batched device calls: parse,
 * fragment-and-serialise, reassemble.
 *
 *   Go (reference)                                            C ABI
 *   --------------------------------------------------------  -------------------------------------
 *   (*UDPMessage).HeaderSize / Size        proxy.go:169-176    hyobfs_udp_header_size
 *   (*UDPMessage).Serialize, varintPut     proxy.go:178-191,   hyobfs_udp_serialize
 *                                                   227-256
 *   ParseUDPMessage                        proxy.go:193-223    hyobfs_udp_parse, hyobfs_udp_parse_batch (device)
 *   FragUDPMessage                         frag.go:7-34        hyobfs_udp_frag_plan
 *   sendMessageAutoFrag + SendMessage      server/udp.go:218-  hyobfs_udp_send_frags,
 *                                          235, server.go:387  hyobfs_udp_frag_batch (device)
 *   (*Defragger).Feed                      frag.go:47-80       hyobfs_udp_defragger_new / _free / _feed,
 *                                                              hyobfs_udp_assemble_batch (device: the copy)
 *
 * The UDP session managers, idle cleanup, the TrafficLogger and the per-session
 * ACL decision cache (core/server/udp.go:237-357) stay with the caller, as does
 * drawing the random PacketID (a salt is the caller's too).
 *
 * WIRE FORMAT (proxy.go:151-158)
 *     SessionID u32 BE | PacketID u16 BE | FragID u8 | FragCount u8 |
 *     varint(len(Addr)) | Addr | Data
 * The varint is quicvarint (RFC 9000 section 16).  varintPut writes the minimal
 * form (1 byte up to 63, 2 up to 16383, 4 up to 2^30 - 1, else 8);
 * quicvarint.Read accepts every form.
 *
 * THE RULES
 *
 *  S. HeaderSize = 8 + varint length + len(Addr); Size = HeaderSize +
 *     len(Data).  Serialize returns -1 when cap < Size and makes no other
 *     check: any address length serialises.
 *
 *  P. ParseUDPMessage, checked in this order:
 *     P1. fewer than 8 bytes: TRUNCATED.
 *     P2. no byte at [8], or fewer than 1 << (b[8] >> 6) varint bytes: TRUNCATED.
 *     P3. varint value 0 or above 2048 (as a 64-bit value): ADDR_LEN.
 *     P4. bytes left after the varint <= the address length: MSG_LEN (at
 *         least one data byte is required).
 *     P5. otherwise OK; the address and the data are offsets into the datagram.
 *     FragID and FragCount are not validated here.
 *
 *  F. FragUDPMessage(m, maxSize).  Size <= maxSize: one message, as it is (its
 *     PacketID, FragID and FragCount are kept).  Otherwise maxPayload =
 *     maxSize - HeaderSize; maxPayload <= 0 returns nothing (NO_ROOM);
 *     otherwise count = ceil(len(Data) / maxPayload), and fragment k carries
 *     Data[k * maxPayload, min(len, (k + 1) * maxPayload)) with FragID = k,
 *     FragCount = count and every other field copied.
 *     TRAP: count is a uint8 in the reference; above 255 it wraps and the
 *     reference then indexes out of range.  The library returns
 *     HYOBFS_UDP_ERR_FRAG_COUNT and produces nothing.
 *
 *  A. sendMessageAutoFrag + SendMessage: what hyobfs_udp_send_frags and
 *     hyobfs_udp_frag_batch reproduce.
 *     A1. Size > 4096 (MaxUDPSize, the size of msgBuf): Serialize returns -1 and
 *         the message is SILENTLY DROPPED; fragmentation is never tried although
 *         it would have fit.  Status TOO_LARGE, zero datagrams.
 *     A2. Size <= max_size: one datagram with PacketID 0, FragID 0, FragCount 1.
 *     A3. otherwise PacketID is the caller's (the reference draws
 *         uint16(rand.Intn(0xFFFF)) + 1 per message) and rule F applies;
 *         maxPayload <= 0 gives NO_ROOM, zero datagrams.
 *     STATED ASSUMPTION: quic-go's SendDatagram is taken to fail with
 *     DatagramTooLargeError exactly when the datagram is longer than the
 *     connection's maximum datagram payload, which is what max_size stands for.
 *
 *  D. Defragger.Feed, an index-level state machine on the host:
 *     D1. FragCount <= 1: the message is returned (WHOLE) and the state is left
 *         untouched; an assembly in progress survives.
 *     D2. FragID >= FragCount: nothing (ERR_FRAG_ID), the state untouched.
 *     D3. a PacketID other than the current one, or a FragCount other than the
 *         current slot count (initially 0 slots): the state is reset and this
 *         fragment stored.
 *     D4. a filled slot is ignored: the first copy wins.
 *     D5. when the last slot fills, the result is the concatenation in FragID
 *         order, and carries the SessionID and Addr of the fragment that
 *         ARRIVED LAST, not of fragment 0.
 *     D6. TRAP: the state is NOT cleared on completion: later fragments with
 *         the same PacketID and FragCount are swallowed by D4 until something
 *         else resets it.
 *
 * Plain C ABI: pointers, sizes, integer status codes.  Additive to ABI 4.
 */
#ifndef HYOBFS_UDPMSG_H
#define HYOBFS_UDPMSG_H

#include <stddef.h>
#include <stdint.h>

#include "hyobfs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HYOBFS_UDP_MAX_SIZE 4096 /* MaxUDPSize, proxy.go:24 */
#define HYOBFS_UDP_MAX_ADDR 2048 /* MaxMessageLength, proxy.go:20 */
#define HYOBFS_UDP_MAX_FRAGS 255 /* FragCount is a uint8 */

/* status, continuing after HYOBFS_SNIFF_ERR_UNRECOGNIZED (-67) */
#define HYOBFS_UDP_ERR_TRUNCATED (-68)  /* P1, P2 */
#define HYOBFS_UDP_ERR_ADDR_LEN (-69)   /* P3 */
#define HYOBFS_UDP_ERR_MSG_LEN (-70)    /* P4 */
#define HYOBFS_UDP_ERR_FRAG_ID (-71)    /* D2 */
#define HYOBFS_UDP_TOO_LARGE (-72)      /* A1: dropped by the reference */
#define HYOBFS_UDP_NO_ROOM (-73)        /* F / A3: max_size <= HeaderSize */
#define HYOBFS_UDP_ERR_FRAG_COUNT (-74) /* F: more than 255 fragments */
#define HYOBFS_UDP_ERR_CAP (-75)        /* an output does not hold the result */
#define HYOBFS_UDP_ERR_PLAN (-76)       /* assemble: a fragment list that cannot be assembled */

/* what hyobfs_udp_defragger_feed returns besides HYOBFS_UDP_ERR_FRAG_ID */
#define HYOBFS_UDP_PENDING 0
#define HYOBFS_UDP_WHOLE 1
#define HYOBFS_UDP_COMPLETE 2

/* the eight fixed bytes of a message */
typedef struct hyobfs_udp_header {
    uint32_t session_id;
    uint16_t packet_id;
    uint8_t frag_id;
    uint8_t frag_count;
} hyobfs_udp_header; /* 8 bytes */

/* one parsed datagram (rule P); offsets are relative to the datagram.  Every
   field but status is 0 when status is not HYOBFS_OK. */
typedef struct hyobfs_udp_parsed {
    int32_t status;
    uint32_t session_id;
    uint16_t packet_id;
    uint8_t frag_id;
    uint8_t frag_count;
    uint32_t addr_off;
    uint32_t addr_len;
    uint32_t data_off;
    uint32_t data_len;
    uint32_t reserved_;
} hyobfs_udp_parsed; /* 32 bytes */

/* one message to send (rule A): its address is addrs[addr_off, +addr_len) of a
   byte buffer, and many messages may share one address */
typedef struct hyobfs_udp_meta {
    uint32_t session_id;
    uint16_t packet_id; /* the caller's draw; used only when the message is fragmented (A3) */
    uint16_t reserved_;
    uint32_t max_size;  /* the connection's maximum datagram payload */
    uint32_t addr_len;
    uint64_t addr_off;
} hyobfs_udp_meta; /* 24 bytes */

/* ---------------------------------------------------------------- host, scalar */

/* HeaderSize (rule S); UINT32_MAX where the sum does not fit 32 bits */
uint32_t hyobfs_udp_header_size(uint32_t addr_len);

/* Serialize (rule S): the bytes written, or -1 when cap < Size.  addr / data may
   be null when their length is 0. */
int64_t hyobfs_udp_serialize(const hyobfs_udp_header* hdr, const uint8_t* addr, uint32_t addr_len, const uint8_t* data,
                             uint32_t data_len, uint8_t* out, size_t cap);

/* ParseUDPMessage (rule P): the status, which is also out->status.  `in` may be
   null when len is 0. */
int hyobfs_udp_parse(const uint8_t* in, size_t len, hyobfs_udp_parsed* out);

/* FragUDPMessage's arithmetic (rule F): HYOBFS_OK with *count fragments of at
   most *max_payload data bytes each (one fragment holding all the data when the
   message fits), or HYOBFS_UDP_NO_ROOM / HYOBFS_UDP_ERR_FRAG_COUNT with both 0. */
int hyobfs_udp_frag_plan(uint32_t addr_len, uint32_t data_len, uint32_t max_size, uint32_t* count,
                         uint32_t* max_payload);

/* Rule A for one message: its datagrams back to back in out[0, cap), their
   lengths in dgram_len[0, *count) (room for HYOBFS_UDP_MAX_FRAGS).  HYOBFS_OK,
   or HYOBFS_UDP_TOO_LARGE / _NO_ROOM / _ERR_FRAG_COUNT / _ERR_CAP (cap too
   small) with *count = 0 and nothing written to out.  The address is addr[0,
   meta->addr_len); meta->addr_off is not used here. */
int hyobfs_udp_send_frags(const hyobfs_udp_meta* meta, const uint8_t* addr, const uint8_t* data, uint32_t data_len,
                          uint8_t* out, size_t cap, uint32_t* dgram_len, uint32_t* count);

/* Defragger (rule D).  It never touches payload bytes: a fragment is known by
   the caller's tag (its batch index, say).  _feed returns
     HYOBFS_UDP_WHOLE      (D1)  tags_out[0] = tag, *n_out = 1
     HYOBFS_UDP_COMPLETE   (D5)  tags_out[0, *n_out) = the fragments' tags in
                                 FragID order; SessionID and Addr are those of
                                 the message just fed
     HYOBFS_UDP_PENDING          *n_out = 0
     HYOBFS_UDP_ERR_FRAG_ID (D2) *n_out = 0
   and HYOBFS_ERR_INVALID for a null argument or a message whose status is not
   HYOBFS_OK.  tags_out has room for HYOBFS_UDP_MAX_FRAGS tags. */
typedef struct hyobfs_udp_defragger hyobfs_udp_defragger;
hyobfs_udp_defragger* hyobfs_udp_defragger_new(void);
void hyobfs_udp_defragger_free(hyobfs_udp_defragger* d);
int hyobfs_udp_defragger_feed(hyobfs_udp_defragger* d, const hyobfs_udp_parsed* m, uint64_t tag, uint64_t* tags_out,
                              uint32_t* n_out);

/* ---------------------------------------------------------------- device, batched
 * All arrays are device memory; calls are asynchronous on `stream`; n == 0
 * (m == 0 for assemble) returns HYOBFS_OK before any pointer is looked at; a
 * null required pointer returns HYOBFS_ERR_INVALID.  Exactly the stated ranges
 * are written and nothing else.
 */

/* Rule P over the datagrams in[in_off[i], +in_len[i]): out[0, n). */
int hyobfs_udp_parse_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint64_t n,
                           hyobfs_udp_parsed* out, void* stream);

/* bytes of device scratch hyobfs_udp_frag_batch needs for n messages (8-aligned) */
uint64_t hyobfs_udp_frag_workspace_size(uint64_t n);

/*
 * Rule A over n messages: message i has the data data[data_off[i],
 * +data_len[i]) and the fields of meta[i].  Its datagrams are packed back to
 * back in `out`, in message order and then fragment order.
 *
 *   status[0, n)   HYOBFS_OK, HYOBFS_UDP_TOO_LARGE, _NO_ROOM, _ERR_FRAG_COUNT
 *                  or _ERR_CAP.
 *   first[0, n]    message i's datagrams are [first[i], first[i + 1]) of
 *                  dgram_off / dgram_len.  Always the numbering of a run with
 *                  enough room, whatever the capacities are.
 *   totals[0, 2)   the bytes and the datagrams the whole batch needs.
 *   dgram_off, dgram_len   entry d (byte offset in `out`, length) for every
 *                  datagram d of a message whose status is HYOBFS_OK.
 *
 * CAPACITY, deterministic.  A message that produces nothing (TOO_LARGE,
 * NO_ROOM, ERR_FRAG_COUNT) adds nothing to either running sum.  Message i is
 * written iff the bytes of messages 0..i are <= out_cap and their datagrams
 * are <= dgram_cap.  Otherwise its status is HYOBFS_UDP_ERR_CAP and nothing of
 * it is written; it still counts in the sums, so every message after it gets
 * HYOBFS_UDP_ERR_CAP too (one that produces nothing included).  `totals`
 * tells the caller what to allocate.  out may be null when out_cap is 0, and
 * dgram_off / dgram_len when dgram_cap is 0 (a sizing run).
 *
 * `workspace`: hyobfs_udp_frag_workspace_size(n) bytes, 8-aligned, not shared
 * with a call that may run at the same time.
 */
int hyobfs_udp_frag_batch(const uint8_t* data, const uint64_t* data_off, const uint32_t* data_len,
                          const hyobfs_udp_meta* meta, const uint8_t* addrs, uint64_t n, uint8_t* out,
                          uint64_t out_cap, uint64_t* dgram_off, uint32_t* dgram_len, uint64_t dgram_cap,
                          uint64_t* first, int32_t* status, uint64_t* totals, void* workspace, void* stream);

/*
 * The copy of Defragger.Feed (D5) over m messages.  parsed[0, n) are the
 * records hyobfs_udp_parse_batch left for the datagrams in[in_off[i], ...).
 * Message j is the concatenation of the data slices of the datagrams
 * frag_idx[msg_first[j] .. msg_first[j + 1]), in that order, written at
 * out + out_off[j]; out_len[j] is the sum of the slice lengths.  A WHOLE
 * message is a list of one.
 *   HYOBFS_UDP_ERR_CAP   the sum exceeds out_cap[j]
 *   HYOBFS_UDP_ERR_PLAN  an empty list, a list longer than 255, an index >= n,
 *                        or a datagram whose parsed status is not HYOBFS_OK
 * Both write nothing of the message and set out_len[j] = 0.
 * out, out_off and out_len are then the packets, off and len that
 * hyobfs_quic_sniff_batch takes.
 */
int hyobfs_udp_assemble_batch(const uint8_t* in, const uint64_t* in_off, const hyobfs_udp_parsed* parsed, uint64_t n,
                              const uint32_t* frag_idx, const uint64_t* msg_first, uint64_t m, uint8_t* out,
                              const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYOBFS_UDPMSG_H */
