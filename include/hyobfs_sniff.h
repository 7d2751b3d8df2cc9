/*
 * hyobfs_sniff.h -- the protocol sniffer (apernet/hysteria
 * extras/sniff/sniff.go): TLS ClientHello server names, HTTP request hosts and
 * Sniffer.TCP's dispatch between the two, batched on the GPU.
 *
 *   Go (reference)                                        C ABI
 *   ----------------------------------------------------  ------------------------------------------
 *   utls.UnmarshalClientHello(pl).ServerName              hyobfs_tls_client_hello_sni_batch (device)
 *     behind len(pl) >= 4 && pl[0] == 0x01  sniff.go:161
 *   (*Sniffer).isTLS(buf)                 sniff.go:59-65  hyobfs_tls_record_sni_batch (device)
 *   (*Sniffer).TCP, the TLS branch        sniff.go:128-144
 *   (*Sniffer).UDP(data, reqAddr)         sniff.go:159-174 hyobfs_quic_sniff_batch (device):
 *     quicInternal.ReadCryptoPayload      payload.go:21-60   hyobfs_quic_read_crypto_payload_batch,
 *     utls.UnmarshalClientHello                              then the ClientHello kernel on its output
 *   (*Sniffer).isHTTP(buf)                sniff.go:46-57  hyobfs_http_request_host_batch (device)
 *   (*Sniffer).TCP, the HTTP branch       sniff.go:110-127
 *     http.ReadRequest(...).Host, net.SplitHostPort
 *   (*Sniffer).TCP, the whole dispatch    sniff.go:103-156 hyobfs_tcp_sniff_batch (device)
 *
 * What the sniffer does with the name (Check, SplitHostPort / JoinHostPort on
 * the request address) is hyobfs_request.h: hyobfs_sniff_check_batch decides
 * which requests are sniffed and hyobfs_request_rewrite_batch takes `names` and
 * the results of the calls below as they are.  hysteria_amd/sniff.py keeps the
 * host's version of it.
 *
 * THE PARSE RULES.  utls forks Go's crypto/tls clientHelloMsg.unmarshal.  Its
 * source was not at hand when this was written, so the rules below, restated
 * from that function as shipped with Go's standard library, are the
 * specification of these entry points (tests/sni_ref.py restates them in
 * Python and is pinned to the reference's own vectors, sniff_test.go:86,135):
 *
 *    1. Skip 4 bytes (handshake type and a uint24 length, which is NOT checked).
 *    2. Read vers (2 bytes) and random (32 bytes).
 *    3. Read session_id, u8-length-prefixed.
 *    4. Read cipher_suites, u16-length-prefixed; an odd length is malformed.
 *    5. Read compression_methods, u8-length-prefixed.
 *    6. Any read past the end of the input is malformed.
 *    7. If the input ends here: a valid hello with no name.
 *    8. Read extensions, u16-length-prefixed; the block must end exactly at the
 *       end of the input, else malformed.
 *    9. Each extension is a u16 type and a u16-length-prefixed body; a
 *       truncated extension is malformed.
 *   10. A type seen twice is malformed (every type, not only 0).
 *   11. Type 0 (server_name): a u16-length-prefixed name list, non-empty, with
 *       which the extension body must end.  Each entry is a u8 name type and a
 *       u16-length-prefixed, non-empty name.  Entries of a name type other than
 *       0 are skipped; a second entry of type 0 is malformed; a name ending in
 *       '.' is malformed.
 *
 * DIVERGENCE.  The bodies of all other extensions are not inspected.  The
 * reference's parser also rejects a hello whose ALPN, key_share, supported
 * versions or other known extension body is malformed; for such hellos (and
 * only for them) the device reports a name where the reference reports none.
 * One device limit has no reference counterpart: more than
 * HYOBFS_TLS_MAX_EXTENSIONS extensions (HYOBFS_SNIFF_ERR_EXTENSIONS).
 *
 * The first failing check decides the status, in input order; within one
 * extension the order is: truncated header or body (MALFORMED), the extension
 * count (EXTENSIONS), a repeated type (MALFORMED), the server_name body
 * (MALFORMED).  NAME_CAP is reported only for a hello that is valid to its end.
 *
 * THE HTTP RULES.  Go's net/http source was not at hand either; the rules below,
 * restated from net/http.readRequest, net/textproto.readMIMEHeader and
 * net/url.ParseRequestURI as shipped with Go 1.25, are the specification of
 * hyobfs_http_request_host_batch (tests/http_ref.py restates them in Python and
 * is pinned to the reference's own requests, sniff_test.go:47-52, :74-77).  The
 * device reports a name or MALFORMED only where the rule is certain and cheap;
 * every rarer form gets HYOBFS_SNIFF_ERR_HOST, "left to the host": the caller
 * runs its own http.ReadRequest on that stream.
 *
 * The input is msg[0, L), L = min(len, 262144) (sniffMaxHTTPHeaderBytes: the
 * LimitReader never shows ReadRequest more).  A line ends at LF; its content
 * excludes that LF and one CR directly before it.  Complete lines are checked
 * in input order and the first failing check decides.  If no line has failed
 * and the blank line that ends the header block is not inside [0, L): MALFORMED
 * when len >= 262144, else NEED_MORE with need = len + 1.
 *
 *   H0. len < 3, or one of the first three bytes is not an ASCII letter
 *       (isHTTP): NOT_HTTP.
 *   H1. The request line is cut at its first space into method and rest, and
 *       rest at its first space into uri and proto; a missing cut is MALFORMED.
 *   H2. method is empty or holds a byte that is not an RFC 7230 tchar (ALPHA,
 *       DIGIT, !#$%&'*+-.^_`|~): MALFORMED.
 *   H3. proto is not exactly "HTTP/" digit "." digit (8 bytes): MALFORMED.
 *   H4. uri: empty is MALFORMED; "*" is fine; origin form (it begins with '/')
 *       is MALFORMED if any byte is < 0x20 or == 0x7F, or if in the part before
 *       the first '?' a '%' is not followed by two hex digits ("//x/y" is a
 *       path here, not an authority); anything else (absolute form, CONNECT's
 *       authority form): HOST.
 *   H5. Header lines, until an empty one.  The first header line begins with
 *       SP or HT: MALFORMED; a later one does (a folded continuation): HOST.
 *       Trailing SP / HT of the line are dropped.  No ':' in the line:
 *       MALFORMED.  The key is everything before the first ':'; a key byte
 *       that is neither tchar nor a space: MALFORMED.  The value is the rest
 *       without its leading SP / HT; a value byte that is not HT, 0x20-0x7E or
 *       >= 0x80: MALFORMED (so a bare CR fails).  A line with an empty key is
 *       skipped after its value is checked.  A key is one of the headers named
 *       below only when it holds no space and equals the name ASCII
 *       case-insensitively.
 *   H6. After the block.  More than one Host line: MALFORMED.  Then each of
 *       these gives HOST: any Transfer-Encoding line, any Trailer line, more
 *       than one Content-Length line, a Content-Length whose value is not 1 to
 *       18 decimal digits.  No Host line, or one with an empty value: OK with
 *       name_len = 0.
 *   H7. The name is net.SplitHostPort(value)'s host, and the whole value on
 *       its error (no ':'; a '[' first without "]:port" behind it; more than
 *       one ':' outside brackets; a stray '[' or ']').  A non-empty value whose
 *       host part is empty (":8080", "[]:80"): HOST.  A name that ends in '.'
 *       or is shaped like an IP address is reported as it is: what to do with
 *       it is the caller's decision, as for TLS names.
 *
 * DIVERGENCE (HTTP).  HOST is no answer of the reference: it marks the requests
 * whose answer this library leaves to the caller's parser.  For every other
 * status the rules above are meant to agree with ReadRequest; where Go rejects
 * a request for a reason the rules do not state (a Host value with bytes
 * net/http's host validation refuses, a header block past Go's own 1 MiB
 * limit, which lies beyond L), the device reports the value as it stands.
 * The reference rewrites the address only when req.Host is not empty; OK with
 * name_len = 0 is that case.  With an absolute-form uri Go takes the Host from
 * the uri: those requests are HOST here.
 *
 * Plain C ABI: pointers, sizes, integer status codes.
 */
#ifndef HYOBFS_SNIFF_H
#define HYOBFS_SNIFF_H

#include <stddef.h>
#include <stdint.h>

#include "hyobfs.h"
#include "hyobfs_quic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* extensions one hello may carry in the device parser (the list of seen types
   lives in LDS; the reference keeps a Go map) */
#define HYOBFS_TLS_MAX_EXTENSIONS 256

/* per-message status, continuing after HYOBFS_QUIC_ERR_* */
#define HYOBFS_SNIFF_ERR_NOT_HELLO (-54)   /* len < 4 or msg[0] != 0x01, sniff.go:161 */
#define HYOBFS_SNIFF_ERR_MALFORMED (-55)   /* UnmarshalClientHello returns nil */
#define HYOBFS_SNIFF_ERR_NAME_CAP (-56)    /* name_len > name_stride: nothing written, name_len / name_off set */
#define HYOBFS_SNIFF_ERR_EXTENSIONS (-57)  /* more than HYOBFS_TLS_MAX_EXTENSIONS extensions */
#define HYOBFS_SNIFF_ERR_NOT_TLS (-58)     /* tls_record: fewer than 3 bytes or isTLS false, sniff.go:59-65 */
#define HYOBFS_SNIFF_ERR_NEED_MORE (-59)   /* tls_record: fewer than `need` bytes so far, sniff.go:131-143 */
#define HYOBFS_SNIFF_ERR_NO_PAYLOAD (-60)  /* quic_sniff: ReadCryptoPayload failed (qres[i].status says why) */
/* continuing after HYOBFS_ACL_ERR_* (-61 .. -64) */
#define HYOBFS_SNIFF_ERR_NOT_HTTP (-65)    /* http_request_host: fewer than 3 bytes or isHTTP false, sniff.go:46-57 */
#define HYOBFS_SNIFF_ERR_HOST (-66)        /* left to the host: the caller runs its own http.ReadRequest */
#define HYOBFS_SNIFF_ERR_UNRECOGNIZED (-67) /* tcp_sniff: neither isHTTP nor isTLS, sniff.go:153-156 */

typedef struct hyobfs_sniff_result {
    int32_t status;    /* HYOBFS_OK or HYOBFS_SNIFF_ERR_* */
    uint32_t name_len; /* full length of the host name; 0 = a valid hello that carries none */
    uint32_t name_off; /* where the name starts inside the message (0 when name_len == 0) */
    uint32_t need;     /* NEED_MORE only: bytes the caller must have before asking again */
} hyobfs_sniff_result; /* 16 bytes */

/*
 * The batched calls below share these rules.  All arrays are device
 * memory; calls are asynchronous on `stream`; n == 0 returns HYOBFS_OK; a null
 * required pointer returns HYOBFS_ERR_INVALID.  Message i is
 * msgs[off[i], +len[i]).  Its name is written to names[i * name_stride,
 * +name_len) and nowhere else; when name_len > name_stride nothing is written
 * and the status is HYOBFS_SNIFF_ERR_NAME_CAP.  Every status but OK and
 * NAME_CAP leaves name_len and name_off 0.
 */

/* Sniffer.UDP's test and parse of one handshake message (sniff.go:161-165):
   NOT_HELLO when len < 4 or msg[0] != 1, else the rules above over the whole
   message. */
int hyobfs_tls_client_hello_sni_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n,
                                      uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* res,
                                      void* stream);

/*
 * The TLS branch of Sniffer.TCP (sniff.go:128-144) over the first bytes of n
 * TCP streams.  Fewer than 3 bytes, or isTLS false (sniff.go:59-65): NOT_TLS.
 * Fewer than 5 bytes: NEED_MORE with need = 5.  Fewer than 5 + contentLength
 * bytes (the u16 at [3, 5)): NEED_MORE with need = 5 + contentLength.
 * Otherwise exactly msg[5, 5 + contentLength) goes through the rules above,
 * as the reference hands it to UnmarshalClientHello: without the test of
 * sniff.go:161, so a body shorter than 4 bytes is MALFORMED and its first
 * byte is not looked at.  name_off is relative to the whole input (>= 5).
 */
int hyobfs_tls_record_sni_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n,
                                uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* res, void* stream);

/*
 * The HTTP branch of Sniffer.TCP (sniff.go:110-127) over the first bytes of n
 * TCP streams, by rules H0-H7 above.  The name written is the host part of
 * req.Host (sniff.go:116-120), so it can go straight to
 * hyobfs_acl_match_sniffed_batch.  name_off is relative to the whole input.
 * NAME_CAP is reported only for a request that is valid to the end of its
 * header block.
 */
int hyobfs_http_request_host_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n,
                                   uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* res, void* stream);

/*
 * Sniffer.TCP's dispatch (sniff.go:103-156) over the first bytes of n TCP
 * streams, in one launch.  Fewer than 3 bytes: NEED_MORE with need = 3.  isHTTP
 * true: exactly what hyobfs_http_request_host_batch reports.  Else isTLS true:
 * exactly what hyobfs_tls_record_sni_batch reports, need included.  Else:
 * UNRECOGNIZED.
 */
int hyobfs_tcp_sniff_batch(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, uint64_t n, uint8_t* names,
                           uint32_t name_stride, hyobfs_sniff_result* res, void* stream);

/* Device workspace quic_sniff_batch needs for n packets. */
uint64_t hyobfs_quic_sniff_workspace_size(uint64_t n);

/*
 * Sniffer.UDP (sniff.go:159-174) over a batch of client Initial packets:
 * hyobfs_quic_read_crypto_payload_batch with these arguments, unchanged and
 * on the same stream (packets unprotected in place, qres and crypto exactly
 * as that call leaves them), then the ClientHello rules over
 * crypto[crypto_off[i], +qres[i].out_len) for every packet whose
 * qres[i].status is HYOBFS_OK.  The other packets get sres[i].status =
 * HYOBFS_SNIFF_ERR_NO_PAYLOAD and nothing is read from their slot.
 */
int hyobfs_quic_sniff_batch(uint8_t* packets, const uint64_t* off, const uint32_t* len, uint64_t n, uint8_t* crypto,
                            const uint64_t* crypto_off, const uint32_t* crypto_cap, hyobfs_quic_result* qres,
                            uint8_t* names, uint32_t name_stride, hyobfs_sniff_result* sres, void* workspace,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYOBFS_SNIFF_H */
