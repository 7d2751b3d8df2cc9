/*
 * hyobfs_request.h -- what the server does with a new request before it dials
 * (apernet/hysteria core/server/server.go:256-335, 405-406): the TCP request and
 * response framing, Sniffer.Check, and the rewrite of the request address with
 * the name the sniffer found.  Scalar host functions, a device handle for a port
 * union, and four batched device calls.
 *
 *   Go (reference)                                              C ABI
 *   ----------------------------------------------------------  -------------------------------------
 *   ReadTCPRequest     core/internal/protocol/proxy.go:39-67    hyobfs_tcp_request_parse,
 *                                                               hyobfs_tcp_request_parse_batch (device)
 *   WriteTCPRequest    proxy.go:69-84                           hyobfs_tcp_request_build
 *   ReadTCPResponse    proxy.go:93-129                          hyobfs_tcp_response_parse
 *   WriteTCPResponse   proxy.go:131-149                         hyobfs_tcp_response_build,
 *                                                               hyobfs_tcp_response_build_batch (device)
 *   padding.String     protocol/padding.go:17-24                hyobfs_req_padding_fill (rule G: a divergence)
 *   ParsePortUnion, Normalize  extras/utils/portunion.go:21-86  hyobfs_port_union_parse
 *   PortUnion.Contains portunion.go:100-107                     hyobfs_port_union_contains,
 *                                                               hyobfs_portset_new / _free (device)
 *   Sniffer.Check      extras/sniff/sniff.go:67-89              hyobfs_sniff_check,
 *                                                               hyobfs_sniff_check_batch (device)
 *   *reqAddr = net.JoinHostPort(name, port)                     hyobfs_request_rewrite,
 *                      sniff.go:121-125, 146-150, 167-171       hyobfs_request_rewrite_batch (device)
 *
 * On one stream a batch of new TCP streams then runs
 *   request parse -> check -> hyobfs_tcp_sniff_batch over the bytes behind the
 *   request -> rewrite -> hyobfs_addr_parse_batch -> hyobfs_acl_match_batch ->
 *   response rows
 * and only statuses and decisions come back (hysteria_amd/request.py works it).
 *
 * STAYS WITH THE CALLER
 *   - The stream read loop and its deadline (sniff.go:91-102): NEED_MORE says
 *     how many bytes to have before asking again.
 *   - http.ReadRequest for the items the sniffer leaves to the host
 *     (HYOBFS_SNIFF_ERR_HOST, here HYOBFS_REQ_ERR_HOST).
 *   - Dialling, and the copy loops behind it.
 *   - The draw of padding lengths (padding.go:18): lengths are inputs here.
 *   - Request build and response parse on the device: they are the client's
 *     side, and host scalar only.
 *
 * THE RULES.  Where a rule below turns out to differ from Go, Go wins.
 *
 *  V. quicvarint, as hyobfs_udpmsg.h states it: the encoding is 1 << (b[0] >> 6)
 *     bytes long, the value is the rest of b[0] and the bytes behind it,
 *     big-endian.  Every form is accepted on reading, the minimal one is written,
 *     values compare as 64-bit (a length of 2^32 + 14 is not 14).
 *
 *  R. ReadTCPRequest over a stream prefix b[0, len) that begins at the address
 *     length (the frame type 0x401 has been consumed, server.go:241-246).  Checks
 *     in stream order, as a blocking reader meets them:
 *     R1. the address-length varint is incomplete: NEED_MORE, need = the
 *         smallest total that could complete it (1 for len == 0, else its length).
 *     R2. its value is 0 or above 2048: ADDR_LEN, as soon as the varint is whole.
 *     R3. the address is incomplete, or no byte is there for the padding varint:
 *         NEED_MORE, need = the end of the address + 1.
 *     R4. the padding varint is incomplete: NEED_MORE, need = its end.
 *     R5. its value is above 4096: PADDING_LEN.
 *     R6. the padding is incomplete: NEED_MORE, need = the whole request.
 *     R7. OK: addr_off, addr_len, consumed (the whole request); the bytes behind
 *         it, b[consumed, len), are the stream's first payload bytes, which
 *         Sniffer.TCP reads.
 *
 *  Q. WriteTCPRequest: varint 0x401, varint addr_len, the address, varint
 *     pad_len, the padding.  S. WriteTCPResponse: one status byte (0 ok, 1 not),
 *     varint msg_len, the message, varint pad_len, the padding.  As in the
 *     reference no length is validated on writing; only the room limits it.
 *
 *  T. ReadTCPResponse over b[0, len), the scheme of R: no status byte:
 *     NEED_MORE, need = 1.  The message-length varint (from b[1]) incomplete:
 *     NEED_MORE (need = 2 without its first byte).  Its value above 2048:
 *     MSG_LEN.  The message incomplete or no byte for the padding varint:
 *     NEED_MORE, need = the end of the message + 1.  Then as R4-R6.  OK:
 *     ok = (b[0] == 0), msg_off, msg_len, consumed.
 *
 *  G. Padding bytes.  The reference draws paddingChars[rand.Intn(62)] from Go's
 *     global math/rand, a stream that cannot be reproduced here (as with the
 *     salts): a stated DIVERGENCE.  Padding lengths are the caller's; byte k of
 *     item i is paddingChars[g(seed, i, k) % 62] with
 *       paddingChars = "a".."z" "A".."Z" "0".."9"              (padding.go:8)
 *       mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *               x *= 0x94D049BB133111EB; x ^= x >> 31            (SplitMix64's output function)
 *       s = mix(seed + 0x9E3779B97F4A7C15 * (i + 1))
 *       z = mix(s + 0x9E3779B97F4A7C15 * (k / 4 + 1))
 *       g = (z >> (16 * (k % 4))) & 0xFFFF
 *     all in 64-bit wrapping arithmetic: a function of (seed, i, k) only, not of
 *     the launch shape.
 *
 *  U. ParsePortUnion + Normalize.  "all" and "*": one range 0-65535.  The text
 *     is split at ','; a part that contains '-' must split into exactly two at
 *     '-'; each number is ParseUint(.., 10, 16) (rule P of hyobfs_addr.h); a
 *     range with start > end is swapped.  Then the ranges are sorted by (start,
 *     end) and those that overlap or touch (uint32(start) <= uint32(last.end) +
 *     1) are merged.  Anything invalid, the empty text included: UNION.
 *
 *  K. PortUnion.Contains: some range has start <= port <= end.  A nil union
 *     (n_ranges < 0, a null handle) is "all ports" at Check; a non-nil union
 *     without ranges contains nothing.
 *
 *  C. Sniffer.Check(isUDP, reqAddr), in the reference's order:
 *     C1. the first byte is '@': 0.
 *     C2. rule H of hyobfs_addr.h fails: 0.  Its LIMIT holds too: a text longer
 *         than 2048 bytes is 0 and is not read.
 *     C3. !rewrite_domain and rule I says the host is no IP literal: 0 (the
 *         empty host is a domain).
 *     C4. strconv.Atoi(port): one optional '+' or '-', then one or more digits
 *         '0'..'9' and nothing else (no '_', no blank); leading zeros in any
 *         number; the value within [-2^63, 2^63 - 1], else ErrRange: 0.
 *     C5. port16 = uint16(value), the low 16 bits of the two's complement:
 *         "-1" is 65535, "65536" is 0, "65616" is 80.
 *     C6. rule K on the TCP or the UDP union.
 *
 *  W. The rewrite.  Per item: the request address text, check, the sniffer's
 *     name row and result, and an optional gate status_in.
 *     W0. status_in != 0: NO_ADDR; nothing of the item is read.
 *     W1. check == 0: the address unchanged, rewritten = 0.
 *     W2. check != 0, by the sniffer's status:
 *         OK and name_len > 0: JoinHostPort(name, port_text), rewritten = 1.
 *           port_text is what stands behind the address's last ':', verbatim
 *           ("+80" stays "+80"); the name goes in '[' ']' exactly when it holds
 *           a ':' or a '%'.  An address without ':' is
 *           HYOBFS_ADDR_ERR_MISSING_PORT (SplitHostPort's error, sniff.go:121-124;
 *           it cannot happen behind rule C).
 *         OK and name_len == 0: the address unchanged.
 *         HYOBFS_SNIFF_ERR_NEED_MORE, _HOST, _NAME_CAP: HYOBFS_REQ_ERR_HOST; the
 *           caller reads the sniffer's result and waits for more bytes or runs
 *           its own parse.
 *         any other status: the address unchanged.
 *     W3. a result longer than the room: ERR_CAP, nothing written, the needed
 *         length reported.
 *
 * Plain C ABI: pointers, sizes, integer status codes.  Additive to ABI 4.
 */
#ifndef HYOBFS_REQUEST_H
#define HYOBFS_REQUEST_H

#include <stddef.h>
#include <stdint.h>

#include "hyobfs.h"
#include "hyobfs_addr.h"
#include "hyobfs_sniff.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HYOBFS_REQ_FRAME_TYPE 0x401  /* FrameTypeTCPRequest */
#define HYOBFS_REQ_MAX_ADDR 2048     /* MaxAddressLength */
#define HYOBFS_REQ_MAX_MSG 2048      /* MaxMessageLength */
#define HYOBFS_REQ_MAX_PADDING 4096  /* MaxPaddingLength */

/* status, continuing after HYOBFS_ADDR_ERR_FAMILY (-85) */
#define HYOBFS_REQ_ERR_NEED_MORE (-86)   /* R, T: fewer than `need` bytes so far */
#define HYOBFS_REQ_ERR_ADDR_LEN (-87)    /* R2 */
#define HYOBFS_REQ_ERR_PADDING_LEN (-88) /* R5, T */
#define HYOBFS_REQ_ERR_MSG_LEN (-89)     /* T */
#define HYOBFS_REQ_ERR_CAP (-90)         /* W3, response build: the row is too short; nothing written */
#define HYOBFS_REQ_ERR_NO_ADDR (-91)     /* W0: the gate is closed */
#define HYOBFS_REQ_ERR_HOST (-92)        /* W2: left to the host */
#define HYOBFS_REQ_ERR_UNION (-93)       /* U */

typedef struct hyobfs_port_range {
    uint16_t start, end; /* inclusive */
} hyobfs_port_range;

/* ---------------------------------------------------------------- host, scalar
 * Host memory, no device.  A text may be null when its length is 0.  A null
 * output pointer is HYOBFS_ERR_INVALID.  Every output is 0 when the status is
 * not HYOBFS_OK, but *need.
 */

/* Rule R.  *need is set for NEED_MORE only. */
int hyobfs_tcp_request_parse(const uint8_t* b, size_t len, uint32_t* need, uint32_t* addr_off, uint32_t* addr_len,
                             uint32_t* consumed);

/* Rule Q with rule G's padding for (seed, item): the bytes written to out[0, cap), or -1 when cap is too small
   (nothing written). */
int64_t hyobfs_tcp_request_build(const uint8_t* addr, size_t addr_len, uint32_t pad_len, uint64_t seed, uint64_t item,
                                 uint8_t* out, size_t cap);

/* Rule T. */
int hyobfs_tcp_response_parse(const uint8_t* b, size_t len, uint32_t* need, uint8_t* ok, uint32_t* msg_off,
                              uint32_t* msg_len, uint32_t* consumed);

/* Rule S with rule G's padding: as hyobfs_tcp_request_build. */
int64_t hyobfs_tcp_response_build(int ok, const uint8_t* msg, size_t msg_len, uint32_t pad_len, uint64_t seed,
                                  uint64_t item, uint8_t* out, size_t cap);

/* Rule G: out[k] = paddingChars[g(seed, item, k) % 62] for k in [0, len). */
void hyobfs_req_padding_fill(uint64_t seed, uint64_t item, uint8_t* out, size_t len);

/* Rule U: the normalised ranges in ranges[0, *n_ranges).  More than `cap` of them: HYOBFS_REQ_ERR_CAP, nothing
   written, *n_ranges the number needed.  Invalid: HYOBFS_REQ_ERR_UNION (ParsePortUnion returns nil). */
int hyobfs_port_union_parse(const uint8_t* text, size_t len, hyobfs_port_range* ranges, uint32_t cap,
                            uint32_t* n_ranges);

/* Rule K over any list of ranges: 1 or 0.  n_ranges < 0 is the nil union: 1. */
int hyobfs_port_union_contains(const hyobfs_port_range* ranges, int64_t n_ranges, uint16_t port);

/* Rule C: 1 or 0.  n_tcp / n_udp < 0 is a nil union. */
int hyobfs_sniff_check(const uint8_t* text, size_t len, int is_udp, int rewrite_domain, const hyobfs_port_range* tcp,
                       int64_t n_tcp, const hyobfs_port_range* udp, int64_t n_udp);

/* Rule W for one address (no gate): the bytes written to out[0, cap), -1 when cap is too small (nothing written),
   HYOBFS_REQ_ERR_HOST or HYOBFS_ADDR_ERR_MISSING_PORT.  sniff_status and name[0, name_len) are the sniffer's. */
int64_t hyobfs_request_rewrite(const uint8_t* addr, size_t addr_len, int check, const uint8_t* name, size_t name_len,
                               int32_t sniff_status, uint8_t* out, size_t cap, uint8_t* rewritten);

/* ---------------------------------------------------------------- the port set
 * Rule K on the device: a map of 65536 bits in device memory, built once from
 * any list of ranges (they need not be normalised), so that a port costs one
 * bit test.  A null handle is the nil union.
 */
typedef struct hyobfs_portset hyobfs_portset;
int hyobfs_portset_new(const hyobfs_port_range* ranges, uint32_t n_ranges, int device, hyobfs_portset** set);
void hyobfs_portset_free(hyobfs_portset* set);

/* ---------------------------------------------------------------- device, batched
 * All arrays are device memory; calls are asynchronous on `stream`; n == 0
 * returns HYOBFS_OK before any pointer is looked at; a null required pointer
 * returns HYOBFS_ERR_INVALID.  Exactly the stated ranges are written and
 * nothing else.  Every output element of every item is written; an item that
 * is not HYOBFS_OK gets zeros everywhere but in status and need (and, for
 * ERR_CAP, out_len).
 */

/*
 * Rule R over the n stream prefixes src[off[i], +len[i]).
 *   status[0, n), need[0, n)
 *   addr_off[0, n)   from src (not from the item); with addr_len it feeds the
 *                    check and the rewrite
 *   rest_off[0, n)   = off[i] + consumed, from src; rest_len = len[i] - consumed:
 *                    they feed hyobfs_tcp_sniff_batch
 */
int hyobfs_tcp_request_parse_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, uint64_t n,
                                   int32_t* status, uint32_t* need, uint64_t* addr_off, uint32_t* addr_len,
                                   uint64_t* rest_off, uint32_t* rest_len, void* stream);

/*
 * Rule C over the n texts src[off[i], +len[i]).  status_in may be null; an item
 * whose status_in is not 0 gets check = 0 and is not read.  `portset` is the
 * union Check would look at (the TCP one for is_udp == 0, the UDP one
 * otherwise; null for nil): is_udp only names which, and must be 0 or 1.
 *   check[0, n)   1 or 0
 */
int hyobfs_sniff_check_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, const int32_t* status_in,
                             uint64_t n, int is_udp, int rewrite_domain, const hyobfs_portset* portset, uint8_t* check,
                             void* stream);

/*
 * Rule W over the n addresses src[off[i], +len[i]), with the sniffer's rows
 * names[i * name_stride, +sres[i].name_len) and results.  status_in may be null.
 * Row i is out[i * out_stride, +out_stride) and is written whole: the text,
 * then zeros (all zeros for NO_ADDR, HOST and MISSING_PORT); an ERR_CAP row is
 * not written at all.
 *   row_off[0, n)     base_off + i * out_stride
 *   out_len[0, n)     the text's length; the needed length for ERR_CAP
 *   rewritten[0, n)   1 where the name went in
 *   status[0, n)
 * `out` (base_off being its offset in the caller's buffer), row_off and out_len
 * are then exactly the src, off and len of hyobfs_addr_parse_batch (give it a
 * length of 0 for the rows whose status is not HYOBFS_OK: an ERR_CAP row holds
 * no text).  out_stride == 0 or out_stride > 2^32 - 16 is HYOBFS_ERR_INVALID,
 * and nothing runs.
 */
int hyobfs_request_rewrite_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, const int32_t* status_in,
                                 const uint8_t* check, const uint8_t* names, uint32_t name_stride,
                                 const hyobfs_sniff_result* sres, uint64_t n, uint8_t* out, uint64_t out_stride,
                                 uint64_t base_off, uint64_t* row_off, uint32_t* out_len, uint8_t* rewritten,
                                 int32_t* status, void* stream);

/*
 * Rule S over n responses.  The message of item i is entry msg_idx[i] of a
 * table of n_msgs texts, msgs[msg_off[m], +msg_len[m]); its padding is pad_len[i]
 * bytes of rule G for (seed, i).  Row i is out[i * out_stride, +out_stride), of
 * which exactly [0, out_len[i]) is written.
 *   status[0, n)    HYOBFS_OK; HYOBFS_REQ_ERR_CAP when the response is longer
 *                   than out_stride (nothing written, out_len the needed
 *                   length); HYOBFS_ERR_INVALID for msg_idx[i] >= n_msgs
 *                   (nothing written, out_len 0)
 * out_len saturates at 2^32 - 1 for an ERR_CAP item whose lengths add up to
 * more.  out_stride > 2^32 - 16 is HYOBFS_ERR_INVALID, and nothing runs.
 */
int hyobfs_tcp_response_build_batch(const uint8_t* ok, const uint32_t* msg_idx, const uint8_t* msgs,
                                    const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n_msgs,
                                    const uint32_t* pad_len, uint64_t seed, uint64_t n, uint8_t* out, uint64_t out_stride,
                                    uint32_t* out_len, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYOBFS_REQUEST_H */
