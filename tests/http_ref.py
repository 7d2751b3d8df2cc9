"""Python restatement of the HTTP branch of Sniffer.TCP and of its dispatch
(extras/sniff/sniff.go:46-57, :103-156) as include/hyobfs_sniff.h states them:
rules H0-H7 over the first bytes of one TCP stream.  Test infrastructure only;
written from the header's rules, not from the kernel.

tests/test_http_sniff.py pins it to the reference's own requests
(sniff_test.go:47-52, :74-77, tests/golden/http_sniff_vectors.json).  Every
function returns the fields of struct hyobfs_sniff_result, (status, name_len,
name_off, need), plus the name.  TLS items go through tests/sni_ref.py.
"""
import sni_ref

OK = 0
MALFORMED, NAME_CAP, NEED_MORE = sni_ref.MALFORMED, sni_ref.NAME_CAP, sni_ref.NEED_MORE
NOT_HTTP, HOST, UNRECOGNIZED = -65, -66, -67
MAX_HEADER_BYTES = 256 * 1024   # sniffMaxHTTPHeaderBytes (sniff.go:21)

_ALPHA = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
_DIGIT = frozenset(b"0123456789")
_TCHAR = _ALPHA | _DIGIT | frozenset(b"!#$%&'*+-.^_`|~")
_HEX = _DIGIT | frozenset(b"abcdefABCDEF")
_WS = b" \t"


class _Decided(Exception):
    def __init__(self, status):
        self.status = status


def is_http(buf: bytes) -> bool:
    """isHTTP (sniff.go:46-57)."""
    return len(buf) >= 3 and all(b in _ALPHA for b in buf[:3])


def split_host(value: bytes):
    """net.SplitHostPort(value): (offset of the host inside value, host), or None
    on its error (then the whole value is the name)."""
    i = value.rfind(b":")
    if i < 0:
        return None                                   # missing port
    j = k = 0
    if value[:1] == b"[":
        end = value.find(b"]")
        if end < 0 or end + 1 == len(value) or end + 1 != i:
            return None                               # missing ']', missing port, too many colons
        at, host = 1, value[1:end]
        j, k = 1, end + 1
    else:
        at, host = 0, value[:i]
        if b":" in host:
            return None                               # too many colons
    if b"[" in value[j:] or b"]" in value[k:]:
        return None
    return at, host


def _request_line(line: bytes):
    """H1-H4."""
    a = line.find(b" ")
    b = line.find(b" ", a + 1) if a >= 0 else -1
    if a < 0 or b < 0:
        raise _Decided(MALFORMED)                     # H1
    method, uri, proto = line[:a], line[a + 1:b], line[b + 1:]
    if not method or any(c not in _TCHAR for c in method):
        raise _Decided(MALFORMED)                     # H2
    if not (len(proto) == 8 and proto[:5] == b"HTTP/" and proto[5] in _DIGIT and proto[6:7] == b"."
            and proto[7] in _DIGIT):
        raise _Decided(MALFORMED)                     # H3
    if not uri:
        raise _Decided(MALFORMED)                     # H4
    if uri == b"*":
        return
    if uri[:1] != b"/":
        raise _Decided(HOST)
    if any(c < 0x20 or c == 0x7F for c in uri):
        raise _Decided(MALFORMED)
    path = uri.split(b"?", 1)[0]
    for i, c in enumerate(path):
        if c == 0x25 and not (i + 2 < len(path) and path[i + 1] in _HEX and path[i + 2] in _HEX):
            raise _Decided(MALFORMED)


def _parse(msg: bytes):
    """H0-H7 over msg: (status, name offset, name, need)."""
    n = len(msg)
    if n < 3 or not is_http(msg):
        return NOT_HTTP, 0, b"", 0                    # H0
    data = msg[:MAX_HEADER_BYTES]
    hosts, clens, coded = [], [], False
    pos, index = 0, 0
    try:
        while True:
            lf = data.find(b"\n", pos)
            if lf < 0:
                if n >= MAX_HEADER_BYTES:
                    return MALFORMED, 0, b"", 0
                return NEED_MORE, 0, b"", n + 1
            end = lf - 1 if lf > pos and data[lf - 1] == 0x0D else lf
            line, start = data[pos:end], pos
            pos, index = lf + 1, index + 1
            if index == 1:
                _request_line(line)
                continue
            if not line:
                break
            if line[0] in _WS:                        # H5
                raise _Decided(MALFORMED if index == 2 else HOST)
            line = line.rstrip(_WS)
            c = line.find(b":")
            if c < 0:
                raise _Decided(MALFORMED)
            key = line[:c]
            if any(x not in _TCHAR and x != 0x20 for x in key):
                raise _Decided(MALFORMED)
            value = line[c + 1:].lstrip(_WS)
            at = start + len(line) - len(value)
            if any(not (x == 9 or 0x20 <= x <= 0x7E or x >= 0x80) for x in value):
                raise _Decided(MALFORMED)
            if not key:
                continue
            name = key.lower()
            if name == b"host":
                hosts.append((at, value))
            elif name == b"content-length":
                clens.append(value)
            elif name in (b"transfer-encoding", b"trailer"):
                coded = True
        if len(hosts) > 1:                            # H6
            raise _Decided(MALFORMED)
        if coded or len(clens) > 1:
            raise _Decided(HOST)
        for v in clens:
            v = v.strip(_WS)
            if not (1 <= len(v) <= 18 and all(x in _DIGIT for x in v)):
                raise _Decided(HOST)
        if not hosts or not hosts[0][1]:
            return OK, 0, b"", 0
        at, value = hosts[0]
        sp = split_host(value)                        # H7
        if sp is None:
            return OK, at, value, 0
        if not sp[1]:
            raise _Decided(HOST)
        return OK, at + sp[0], sp[1], 0
    except _Decided as d:
        return d.status, 0, b"", 0


def http_request_host(msg: bytes, name_stride: int = 255):
    """hyobfs_http_request_host_batch for the first bytes of one stream."""
    st, off, name, need = _parse(msg)
    if st == OK and len(name) > name_stride:
        return NAME_CAP, len(name), off, need, b""
    return st, len(name), off, need, name


def tcp_sniff(msg: bytes, name_stride: int = 255):
    """hyobfs_tcp_sniff_batch for the first bytes of one stream (sniff.go:103-156)."""
    if len(msg) < 3:
        return NEED_MORE, 0, 0, 3, b""
    if is_http(msg):
        return http_request_host(msg, name_stride)
    if sni_ref.is_tls(msg):
        return sni_ref.tls_record_sni(msg, name_stride)
    return UNRECOGNIZED, 0, 0, 0, b""
