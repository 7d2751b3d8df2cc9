"""Python restatement of the ClientHello server-name rules of
include/hyobfs_sniff.h (Go's crypto/tls clientHelloMsg.unmarshal as utls forks
it, restricted to what decides ServerName) and of the sniffer's two front ends
(extras/sniff/sniff.go:59-65, 128-144, 159-174).  Test infrastructure only.

tests/test_sniff.py pins it to the reference's own vectors (sniff_test.go:86,
:135, tests/golden/sniff_vectors.json).  Every function returns the fields of
struct hyobfs_sniff_result: (status, name_len, name_off, need), plus the name.
"""
OK = 0
NOT_HELLO, MALFORMED, NAME_CAP, EXTENSIONS, NOT_TLS, NEED_MORE, NO_PAYLOAD = range(-54, -61, -1)
MAX_EXTENSIONS = 256


class _Malformed(Exception):
    pass


class _Reader:
    """cryptobyte.String: reads fail (malformed) past the end."""

    def __init__(self, data: bytes, pos: int, end: int):
        self.d, self.i, self.end = data, pos, end

    def empty(self):
        return self.i == self.end

    def skip(self, k):
        if self.end - self.i < k:
            raise _Malformed
        self.i += k

    def uint(self, k):
        if self.end - self.i < k:
            raise _Malformed
        v = int.from_bytes(self.d[self.i:self.i + k], "big")
        self.i += k
        return v

    def prefixed(self, k):
        """A k-byte length and that many bytes, as a reader of their own."""
        n = self.uint(k)
        if self.end - self.i < n:
            raise _Malformed
        sub = _Reader(self.d, self.i, self.i + n)
        self.i += n
        return sub


def unmarshal(data: bytes, start: int = 0, end: int | None = None):
    """The parse rules over data[start:end]: (status, name offset in data, name).
    OK with an empty name = a valid hello that carries none."""
    end = len(data) if end is None else end
    try:
        s = _Reader(data, start, end)
        s.skip(4)                       # rule 1: type + uint24 length, unchecked
        s.skip(2 + 32)                  # rule 2
        s.prefixed(1)                   # rule 3
        suites = s.prefixed(2)          # rule 4
        if (suites.end - suites.i) % 2:
            raise _Malformed
        s.prefixed(1)                   # rule 5
        if s.empty():                   # rule 7
            return OK, 0, b""
        ext = s.prefixed(2)             # rule 8
        if not s.empty():
            raise _Malformed
        seen = []
        name_off, name = 0, b""
        while not ext.empty():
            typ = ext.uint(2)           # rule 9
            body = ext.prefixed(2)
            if len(seen) == MAX_EXTENSIONS:
                return EXTENSIONS, 0, b""
            if typ in seen:             # rule 10
                raise _Malformed
            seen.append(typ)
            if typ != 0:
                continue
            lst = body.prefixed(2)      # rule 11
            if lst.empty() or not body.empty():
                raise _Malformed
            while not lst.empty():
                nt = lst.uint(1)
                nm = lst.prefixed(2)
                if nm.empty():
                    raise _Malformed
                if nt != 0:
                    continue
                if name:
                    raise _Malformed
                name_off, name = nm.i, data[nm.i:nm.end]
                if name.endswith(b"."):
                    raise _Malformed
        return OK, name_off, name
    except _Malformed:
        return MALFORMED, 0, b""


def _result(st, off, name, stride, need=0):
    if st == OK and len(name) > stride:
        return NAME_CAP, len(name), off, need, b""
    return st, len(name), off, need, name


def client_hello_sni(msg: bytes, name_stride: int = 255):
    """hyobfs_tls_client_hello_sni_batch for one message (sniff.go:161-165)."""
    if len(msg) < 4 or msg[0] != 1:
        return NOT_HELLO, 0, 0, 0, b""
    return _result(*unmarshal(msg), name_stride)


def is_tls(buf: bytes) -> bool:
    """isTLS (sniff.go:59-65)."""
    return len(buf) >= 3 and 0x16 <= buf[0] <= 0x17 and buf[1] == 3 and buf[2] <= 9


def tls_record_sni(msg: bytes, name_stride: int = 255):
    """hyobfs_tls_record_sni_batch for the first bytes of one stream (sniff.go:128-144)."""
    if not is_tls(msg):
        return NOT_TLS, 0, 0, 0, b""
    need = 5 if len(msg) < 5 else 5 + int.from_bytes(msg[3:5], "big")
    if len(msg) < need:
        return NEED_MORE, 0, 0, need, b""
    return _result(*unmarshal(msg, 5, need), name_stride)


def quic_sniff(payload, name_stride: int = 255):
    """hyobfs_quic_sniff_batch's second half: `payload` is ReadCryptoPayload's
    result, or None when it failed (sniff.go:159-165)."""
    if payload is None:
        return NO_PAYLOAD, 0, 0, 0, b""
    return client_hello_sni(payload, name_stride)
