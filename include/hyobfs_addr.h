/*
 * hyobfs_addr.h -- the request address "host:port" (apernet/hysteria
 * extras/outbounds): the step between the UDP relay message, whose Addr is a
 * text, and the ACL, which takes a name, addresses and a port; and the way
 * back, from the address a reply came from to the Addr text of the message
 * that carries it.  Scalar host functions, and three batched device calls:
 * parse, parse the addresses hyobfs_udp_parse_batch found, format.
 *
 *   Go (reference)                                              C ABI
 *   ----------------------------------------------------------  -------------------------------------
 *   net.SplitHostPort, as called per datagram by                hyobfs_addr_split
 *     udpSessionEntry.Feed -> checkAddr / WriteTo
 *       core/server/udp.go:113-120
 *     PluggableOutboundAdapter.CheckUDP, udpConnAdapter.WriteTo
 *       extras/outbounds/interface.go:113-126, 141-154
 *   parsePortUint16 = strconv.ParseUint(port, 10, 16)           hyobfs_addr_parse_port
 *       interface.go:71-77
 *   tryParseIP = net.ParseIP + To4                              hyobfs_addr_parse_ip
 *       extras/outbounds/utils.go:29-40
 *   all of it, up to HostInfo for aclEngine.handle              hyobfs_addr_parse,
 *       extras/outbounds/acl.go:79-101                          hyobfs_addr_parse_batch (device),
 *                                                               hyobfs_addr_parse_udp_batch (device)
 *   AddrEx{Host: addr.IP.String(), Port}.String() =             hyobfs_addr_format,
 *     net.JoinHostPort(host, strconv.Itoa(port))                hyobfs_addr_format_batch (device)
 *       ob_direct.go:298-308, interface.go:49-51, 132-139;
 *       the Addr that sendMessageAutoFrag serialises,
 *       core/server/udp.go:199-207
 *
 * STAYS WITH THE CALLER
 *   - DNS resolution: a host that is no IP literal gets no address here; the
 *     caller's resolver may overlay ipv4 / ipv6 / ip_flags afterwards.
 *   - The "@" internal addresses: "@SpeedTest" is simply MISSING_PORT here.
 *     (Sniffer.Check, which tests for them, uses strconv.Atoi and has a port
 *     union, and the rewrite of the address are hyobfs_request.h's.)
 *   - The per-session ACL decision cache.
 *   - The SOCKS5 address form of ob_socks5.go.
 *
 * THE RULES.  Go's standard library is not part of the reference tree, so
 * this header is the statement of record of what net.SplitHostPort,
 * strconv.ParseUint, net.ParseIP (netip.ParseAddr) and IP.String do.  Where a
 * rule below turns out to differ from Go, Go wins: the difference is a bug to
 * fix, not a divergence to keep.
 *
 *  H. net.SplitHostPort(text).  Checks in this order, one status per failure.
 *     H1. no ':' in the text (the empty text included): MISSING_PORT.
 *         Let i be the last ':'.
 *         The text begins with '[':
 *           let end be the first ']'; none: MISSING_BRACKET.
 *           end + 1 == len: MISSING_PORT.
 *           end + 1 == i: good.
 *           otherwise TOO_MANY_COLONS when the byte at end + 1 is ':', else
 *           MISSING_PORT.
 *           The host is (1, end); j = 1, k = end + 1.
 *         It does not:
 *           the host is [0, i); a ':' inside it: TOO_MANY_COLONS.  j = k = 0.
 *     H2. a '[' anywhere in [j, len): UNEXPECTED_LBRACKET.
 *     H3. then a ']' anywhere in [k, len): UNEXPECTED_RBRACKET.
 *     The port is [i + 1, len).  An empty host or an empty port passes rule H.
 *
 *  P. strconv.ParseUint(port, 10, 16).  One or more bytes, all '0'..'9', value
 *     at most 65535.  Any number of leading zeros is fine.  No sign, no '_', no
 *     blank.  Everything else (the empty port included) is PORT.  The value is
 *     computed from the digits after the leading zeros, of which more than five
 *     are already too many: a long run of digits cannot wrap.
 *
 *  I. net.ParseIP(host): netip.ParseAddr with any zone refused.  Scan for the
 *     first '.', ':' or '%': '.' first parses as IPv4, ':' first as IPv6; '%'
 *     first, or none of the three, is not an IP.  A '%' anywhere later ends in
 *     "not an IP" as well (the IPv4 parser sees an unexpected character;
 *     ParseIP refuses a zone and ParseAddr an empty one).
 *     IPv4: exactly four fields separated by single '.'; no leading, trailing
 *       or doubled dot; each field is one or more digits with a value of at
 *       most 255; a second digit after a leading '0' is refused ("00", "01").
 *     IPv6: an optional leading "::" (alone: the zero address).  Then groups of
 *       1 to 4 hex digits of either case; a fifth digit is refused.  A group
 *       followed by '.' starts an embedded IPv4: allowed only when a "::" has
 *       been seen or exactly 12 bytes are filled; it needs room for 4 bytes; it
 *       is re-read from the group's first character by the IPv4 rule and must
 *       run to the end of the text.  After a group comes the end, or a ':' that
 *       must be followed by more.  A second ':' there is the "::": at most one;
 *       it may end the text; it must stand for at least one zero group (16
 *       bytes filled together with a "::" is refused).  Fewer than 16 bytes
 *       without "::" is refused.  Bytes left over are refused.
 *     The result is always the 16-byte form, an IPv4 address as ::ffff:a.b.c.d.
 *     The longest text that can pass is 45 bytes (HYOBFS_ADDR_LITERAL_MAX); a
 *     longer host is not an IP and is not looked at.
 *
 *  T. tryParseIP.  Rule I passes: bytes 0-9 zero and bytes 10, 11 ff ff
 *     (To4() != nil) sets ip_flags bit 0 and ipv4 = the last four bytes;
 *     otherwise bit 1 and ipv6 = the 16 bytes.  So "::ffff:1.2.3.4" and
 *     "::ffff:102:304" are IPv4, and "::1.2.3.4" is IPv6.  Rule I does not
 *     pass: no flag; a domain.  In every case the ACL's name is the host text
 *     itself (HostInfo{Name: reqAddr.Host}, acl.go:80), IP literals included.
 *
 *  F. IP.String() + JoinHostPort + Itoa.  Family 4, or family 16 with
 *     To4() != nil: dotted decimal without leading zeros.  Any other 16 bytes:
 *     eight groups in lower-case hex without leading zeros, ':' between them;
 *     "::" replaces the longest run of two or more zero groups, the first one
 *     on equal lengths; a single zero group is written "0".  The host is put in
 *     '[' ']' exactly when it contains a ':'.  Then ':' and the port in
 *     decimal.  The longest result is 47 bytes (HYOBFS_ADDR_FORMAT_MAX).  A
 *     family other than 4 or 16: FAMILY.
 *
 *  LIMIT.  An address longer than HYOBFS_UDP_MAX_ADDR (2048) bytes is TOO_LONG
 *  and nothing of it is read.
 *
 * Plain C ABI: pointers, sizes, integer status codes.  Additive to ABI 4.
 */
#ifndef HYOBFS_ADDR_H
#define HYOBFS_ADDR_H

#include <stddef.h>
#include <stdint.h>

#include "hyobfs.h"
#include "hyobfs_udpmsg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HYOBFS_ADDR_LITERAL_MAX 45 /* rule I: the longest IP literal */
#define HYOBFS_ADDR_FORMAT_MAX 47  /* rule F: "[ffff:...:ffff]:65535" */

/* status, continuing after HYOBFS_UDP_ERR_PLAN (-76) */
#define HYOBFS_ADDR_ERR_NO_ADDR (-77)             /* parse_udp_batch: the datagram did not parse */
#define HYOBFS_ADDR_ERR_MISSING_PORT (-78)        /* H1 */
#define HYOBFS_ADDR_ERR_TOO_MANY_COLONS (-79)     /* H1 */
#define HYOBFS_ADDR_ERR_MISSING_BRACKET (-80)     /* H1 */
#define HYOBFS_ADDR_ERR_UNEXPECTED_LBRACKET (-81) /* H2 */
#define HYOBFS_ADDR_ERR_UNEXPECTED_RBRACKET (-82) /* H3 */
#define HYOBFS_ADDR_ERR_PORT (-83)                /* P */
#define HYOBFS_ADDR_ERR_TOO_LONG (-84)            /* LIMIT */
#define HYOBFS_ADDR_ERR_FAMILY (-85)              /* F */

/* ip_flags, as hyobfs_acl.h takes them */
#define HYOBFS_ADDR_HAS_IPV4 1
#define HYOBFS_ADDR_HAS_IPV6 2

/* ---------------------------------------------------------------- host, scalar
 * Host memory, no device.  `text` may be null when len is 0.  A null output
 * pointer is HYOBFS_ERR_INVALID.  Every output is 0 when the status is not
 * HYOBFS_OK.
 */

/* net.SplitHostPort (rule H, and the LIMIT): offsets (from text) and lengths of
   the host and the port, or the status. */
int hyobfs_addr_split(const uint8_t* text, size_t len, uint32_t* host_off, uint32_t* host_len, uint32_t* port_off,
                      uint32_t* port_len);

/* parsePortUint16 (rule P, interface.go:71-77): HYOBFS_OK and *port, or HYOBFS_ADDR_ERR_PORT. */
int hyobfs_addr_parse_port(const uint8_t* text, size_t len, uint16_t* port);

/* net.ParseIP (rule I): 1 and the 16-byte form in ip16, or 0 (ip16 zeroed). */
int hyobfs_addr_parse_ip(const uint8_t* text, size_t len, uint8_t* ip16);

/* Rules H, P and T in one call (CheckUDP / WriteTo up to the HostInfo of
   aclEngine.handle): the name is text[*name_off, +*name_len); ipv4 is 4 bytes,
   ipv6 16, *ip_flags HYOBFS_ADDR_HAS_IPV4 / _IPV6 or 0. */
int hyobfs_addr_parse(const uint8_t* text, size_t len, uint32_t* name_off, uint32_t* name_len, uint8_t* ipv4,
                      uint8_t* ipv6, uint8_t* ip_flags, uint16_t* port);

/* AddrEx.String() of {IP.String(), port} (rule F): ip is 16 bytes for family 16
   and 4 for family 4.  The bytes written to out[0, cap) (no terminator), -1 when
   cap is too small (nothing written), or HYOBFS_ADDR_ERR_FAMILY. */
int hyobfs_addr_format(const uint8_t* ip, uint32_t family, uint16_t port, uint8_t* out, size_t cap);

/* ---------------------------------------------------------------- device, batched
 * All arrays are device memory; calls are asynchronous on `stream`; n == 0
 * returns HYOBFS_OK before any pointer is looked at; a null required pointer
 * returns HYOBFS_ERR_INVALID.  Exactly the stated ranges are written and
 * nothing else.
 */

/*
 * Rules H, P and T over the n texts src[off[i], +len[i]).
 *   status[0, n)      HYOBFS_OK or one of the statuses above
 *   name_off[0, n)    the host's offset from src (not from the item)
 *   name_len[0, n)
 *   ipv4[0, 4n), ipv6[0, 16n), ip_flags[0, n), port[0, n)
 * Every output element of every item is written; an item whose status is not
 * HYOBFS_OK gets zeros everywhere but in status.  `src` (as names) and these
 * arrays are exactly the arguments of hyobfs_acl_match_batch.
 */
int hyobfs_addr_parse_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, uint64_t n, int32_t* status,
                            uint64_t* name_off, uint32_t* name_len, uint8_t* ipv4, uint8_t* ipv6, uint8_t* ip_flags,
                            uint16_t* port, void* stream);

/*
 * The same over the addresses hyobfs_udp_parse_batch found: item i is
 * in[in_off[i] + parsed[i].addr_off, +parsed[i].addr_len).  parsed[i].status
 * != HYOBFS_OK gives HYOBFS_ADDR_ERR_NO_ADDR, and nothing of that datagram is
 * read.  name_off is the offset from `in`.
 */
int hyobfs_addr_parse_udp_batch(const uint8_t* in, const uint64_t* in_off, const hyobfs_udp_parsed* parsed, uint64_t n,
                                int32_t* status, uint64_t* name_off, uint32_t* name_len, uint8_t* ipv4, uint8_t* ipv6,
                                uint8_t* ip_flags, uint16_t* port, void* stream);

/*
 * Rule F over n addresses: ip is 16 bytes per item (family 4: its first four),
 * family one byte per item, port a uint16.  Row i is out[i * out_stride,
 * +out_stride) and is written whole: the text, then zeros; all zeros for a
 * FAMILY item.  out_stride < HYOBFS_ADDR_FORMAT_MAX is HYOBFS_ERR_INVALID, and
 * nothing runs.
 *   out_len[0, n)   the text's length (0 for a FAMILY item)
 *   status[0, n)    HYOBFS_OK or HYOBFS_ADDR_ERR_FAMILY
 *   meta            optional (may be null): for an item whose status is
 *                   HYOBFS_OK, meta[i].addr_off = base_off + i * out_stride and
 *                   meta[i].addr_len = the text's length.  The other fields, and
 *                   the items that failed, are left as they are.
 * `out` (as addrs, base_off being its offset there) and `meta` then feed
 * hyobfs_udp_frag_batch directly.
 */
int hyobfs_addr_format_batch(const uint8_t* ip, const uint8_t* family, const uint16_t* port, uint64_t n, uint8_t* out,
                             uint64_t out_stride, uint64_t base_off, uint32_t* out_len, hyobfs_udp_meta* meta,
                             int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYOBFS_ADDR_H */
