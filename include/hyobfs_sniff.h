/*
 * hyobfs_sniff.h -- the protocol sniffer's TLS ClientHello server-name
 * extraction (apernet/hysteria extras/sniff/sniff.go), batched on the GPU.
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
 *
 * What the sniffer does with the name (Check, SplitHostPort / JoinHostPort on
 * the request address) stays on the host: hysteria_amd/sniff.py shows it.  The
 * HTTP branch of Sniffer.TCP (net/http ReadRequest) is not covered.
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

typedef struct hyobfs_sniff_result {
    int32_t status;    /* HYOBFS_OK or HYOBFS_SNIFF_ERR_* */
    uint32_t name_len; /* full length of the host name; 0 = a valid hello that carries none */
    uint32_t name_off; /* where the name starts inside the message (0 when name_len == 0) */
    uint32_t need;     /* tls_record only: bytes the caller must have before asking again */
} hyobfs_sniff_result; /* 16 bytes */

/*
 * The three batched calls below share these rules.  All arrays are device
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
