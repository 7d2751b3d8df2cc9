"""The request address "host:port" -- what ``extras/outbounds`` does with it per
datagram, on MI355X.

==================================================  ==================================================
reference (Go)                                      here
==================================================  ==================================================
``net.SplitHostPort`` in ``CheckUDP`` / ``WriteTo``  ``split_host_port``
(interface.go:113-126, 141-154)
``parsePortUint16`` (interface.go:71-77)            ``parse_port``
``tryParseIP`` (utils.go:29-40)                     ``parse_ip``
all of it, up to ``HostInfo`` (acl.go:79-101)       ``parse``, ``parse_batch`` and
                                                    ``parse_udp_batch`` (GPU)
``AddrEx.String()`` of a reply's address            ``format`` and ``format_batch`` (GPU)
(interface.go:49-51, ob_direct.go:298-308)
``Feed`` -> ``checkAddr`` -> ``aclEngine.handle``   ``relay_acl_decisions``
==================================================  ==================================================

``include/hyobfs_addr.h`` states the rules.  Everything runs in ``libhyobfs.so``;
there is no Python path.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._dev import _pack, _ptr, _records, _stream, _to

LITERAL_MAX, FORMAT_MAX, MAX_ADDR = 45, 47, 2048
HAS_IPV4, HAS_IPV6 = 1, 2
(ERR_NO_ADDR, ERR_MISSING_PORT, ERR_TOO_MANY_COLONS, ERR_MISSING_BRACKET, ERR_UNEXPECTED_LBRACKET,
 ERR_UNEXPECTED_RBRACKET, ERR_PORT, ERR_TOO_LONG, ERR_FAMILY) = range(-77, -86, -1)
ERRORS = {
    ERR_NO_ADDR: "the datagram has no address",
    ERR_MISSING_PORT: "missing port in address",
    ERR_TOO_MANY_COLONS: "too many colons in address",
    ERR_MISSING_BRACKET: "missing ']' in address",
    ERR_UNEXPECTED_LBRACKET: "unexpected '[' in address",
    ERR_UNEXPECTED_RBRACKET: "unexpected ']' in address",
    ERR_PORT: "invalid port",
    ERR_TOO_LONG: "address too long",
    ERR_FAMILY: "address family is neither 4 nor 16",
}
STATUS_NAMES = {
    _lib.HYOBFS_OK: "OK", ERR_NO_ADDR: "NO_ADDR", ERR_MISSING_PORT: "MISSING_PORT",
    ERR_TOO_MANY_COLONS: "TOO_MANY_COLONS", ERR_MISSING_BRACKET: "MISSING_BRACKET",
    ERR_UNEXPECTED_LBRACKET: "UNEXPECTED_LBRACKET", ERR_UNEXPECTED_RBRACKET: "UNEXPECTED_RBRACKET", ERR_PORT: "PORT",
    ERR_TOO_LONG: "TOO_LONG", ERR_FAMILY: "FAMILY",
}


class AddrError(ValueError):
    def __init__(self, status: int):
        self.status = status
        super().__init__(f"{ERRORS.get(status, 'error')} ({status})")


def _adlib(lib=None):
    return _lib.declare(lib or _lib.load(), "addr", _lib._ADDR_SIG)


def _buf(b: bytes):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def _bytes(text) -> bytes:
    return text.encode("utf-8", "surrogateescape") if isinstance(text, str) else bytes(text)


# ------------------------------------------------------------------ host, scalar
def split_record(text) -> tuple[int, int, int, int, int]:
    """hyobfs_addr_split: (status, host_off, host_len, port_off, port_len)."""
    t = _bytes(text)
    b = _buf(t)
    v = [ctypes.c_uint32() for _ in range(4)]
    st = _adlib().hyobfs_addr_split(ctypes.addressof(b), len(t), *(ctypes.byref(x) for x in v))
    return (st, *(x.value for x in v))


def split_host_port(text) -> tuple[bytes, bytes]:
    """net.SplitHostPort: (host, port) as bytes; AddrError where it returns an error."""
    t = _bytes(text)
    st, ho, hl, po, pl = split_record(t)
    if st != _lib.HYOBFS_OK:
        raise AddrError(st)
    return t[ho:ho + hl], t[po:po + pl]


def parse_port(text) -> int:
    """parsePortUint16; AddrError(ERR_PORT) where it returns an error."""
    t = _bytes(text)
    b = _buf(t)
    v = ctypes.c_uint16()
    st = _adlib().hyobfs_addr_parse_port(ctypes.addressof(b), len(t), ctypes.byref(v))
    if st != _lib.HYOBFS_OK:
        raise AddrError(st)
    return v.value


def parse_ip(text):
    """net.ParseIP: the 16-byte form, or None."""
    t = _bytes(text)
    b = _buf(t)
    out = (ctypes.c_uint8 * 16)()
    ok = _adlib().hyobfs_addr_parse_ip(ctypes.addressof(b), len(t), ctypes.addressof(out))
    return bytes(out) if ok == 1 else None


def parse_record(text) -> tuple[int, int, int, bytes, bytes, int, int]:
    """hyobfs_addr_parse: (status, name_off, name_len, ipv4, ipv6, ip_flags, port)."""
    t = _bytes(text)
    b = _buf(t)
    no, nl, fl, port = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint16()
    v4, v6 = (ctypes.c_uint8 * 4)(), (ctypes.c_uint8 * 16)()
    st = _adlib().hyobfs_addr_parse(ctypes.addressof(b), len(t), ctypes.byref(no), ctypes.byref(nl), ctypes.addressof(v4),
                                    ctypes.addressof(v6), ctypes.byref(fl), ctypes.byref(port))
    return st, no.value, nl.value, bytes(v4), bytes(v6), fl.value, port.value


def parse(text):
    """CheckUDP's view of one address: (name, ipv4 or None, ipv6 or None, port);
    AddrError where the reference returns an error."""
    t = _bytes(text)
    st, no, nl, v4, v6, fl, port = parse_record(t)
    if st != _lib.HYOBFS_OK:
        raise AddrError(st)
    return t[no:no + nl], v4 if fl & HAS_IPV4 else None, v6 if fl & HAS_IPV6 else None, port


def format(ip: bytes, port: int, cap: int = FORMAT_MAX):   # noqa: A001 (the name the reference's step has)
    """AddrEx.String() of a 4- or 16-byte address and a port: the text as bytes, -1
    when ``cap`` is too small; AddrError(ERR_FAMILY) for another length."""
    ip = bytes(ip)
    b, out = _buf(ip.ljust(16, b"\0")), (ctypes.c_uint8 * max(cap, 1))()
    n = _adlib().hyobfs_addr_format(ctypes.addressof(b), len(ip), port, ctypes.addressof(out), cap)
    if n == ERR_FAMILY:
        raise AddrError(n)
    return -1 if n < 0 else bytes(out[:n])


# ------------------------------------------------------------------ device batches
def parse_batch(src, off, len_, n: int, status, name_off, name_len, ipv4, ipv6, ip_flags, port, stream=None) -> None:
    """hyobfs_addr_parse_batch: text i is src[off[i], +len_[i]).  ``src`` (as names)
    and the outputs are the arguments of ``RuleSet.match_batch``."""
    st = _adlib().hyobfs_addr_parse_batch(_ptr(src), _ptr(off), _ptr(len_), n, _ptr(status), _ptr(name_off),
                                          _ptr(name_len), _ptr(ipv4), _ptr(ipv6), _ptr(ip_flags), _ptr(port),
                                          _stream(stream, status))
    _lib.check(st, "addr_parse_batch")


def parse_udp_batch(in_, in_off, parsed, n: int, status, name_off, name_len, ipv4, ipv6, ip_flags, port,
                    stream=None) -> None:
    """hyobfs_addr_parse_udp_batch: the addresses ``udpmsg.parse_batch`` found."""
    st = _adlib().hyobfs_addr_parse_udp_batch(_ptr(in_), _ptr(in_off), _ptr(parsed), n, _ptr(status), _ptr(name_off),
                                              _ptr(name_len), _ptr(ipv4), _ptr(ipv6), _ptr(ip_flags), _ptr(port),
                                              _stream(stream, status))
    _lib.check(st, "addr_parse_udp_batch")


def format_batch(ip, family, port, n: int, out, out_stride: int, base_off: int, out_len, meta, status,
                 stream=None) -> None:
    """hyobfs_addr_format_batch: row i of ``out`` gets the text of (ip[16 i, +16),
    port[i]); ``meta`` (may be None) gets addr_off / addr_len for ``udpmsg.frag_batch``."""
    st = _adlib().hyobfs_addr_format_batch(_ptr(ip), _ptr(family), _ptr(port), n, _ptr(out), out_stride, base_off,
                                           _ptr(out_len), _ptr(meta), _ptr(status), _stream(stream, status))
    _lib.check(st, "addr_format_batch")


def parse_outputs(n: int, dev):
    """The seven output tensors of the parse calls for n items on ``dev``: status,
    name_off, name_len, ipv4, ipv6, ip_flags, port (int16: torch has no uint16 arithmetic; the bits are the port's)."""
    import torch
    return (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(4 * n, dtype=torch.uint8, device=dev),
            torch.zeros(16 * n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
            torch.zeros(n, dtype=torch.int16, device=dev))


def relay_acl_decisions(rules, datagrams, device: int = 0):
    """The relay-to-decision chain, worked: ``udpmsg.parse_batch``,
    ``parse_udp_batch`` and ``RuleSet.match_batch`` on one stream over a list of
    relay datagrams; neither the addresses nor what is parsed out of them leave
    the device.  Returns per datagram (outbound, hijack address or None), or None
    where the message or its address is refused.  Only the statuses, the ACL's
    results and the names the ACL leaves to the host (ERR_HOST) are copied back;
    those are finished by ``match_host`` with what the device parsed."""
    import torch

    from . import acl, udpmsg
    n = len(datagrams)
    if n == 0:
        return []
    dev = torch.device("cuda", device)
    stream = torch.cuda.current_stream(dev)
    buf, off, lens = _pack(datagrams)
    d_in, d_off, d_len = _to(dev, buf), _to(dev, off), _to(dev, lens)
    d_parsed = torch.zeros(n * udpmsg.PARSED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_st, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port = parse_outputs(n, dev)
    d_res = torch.zeros(n * acl.ACL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_proto = torch.full((n,), acl.PROTO_UDP, dtype=torch.uint8, device=dev)
    udpmsg.parse_batch(d_in, d_off, d_len, n, d_parsed, stream=stream)
    parse_udp_batch(d_in, d_off, d_parsed, n, d_st, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port, stream=stream)
    # an item without an address is an empty name, no address and port 0 to the ACL; its result is not used
    rules.match_batch(d_in, d_noff, d_nlen, d_v4, d_v6, d_fl, d_proto, d_port, n, d_res, stream=stream, device=device)
    st = d_st.cpu().numpy()
    res = _records(d_res, acl.ACL_RESULT_DTYPE)
    left = [i for i in range(n) if st[i] == _lib.HYOBFS_OK and res[i]["status"] == acl.ERR_HOST]
    host = {}
    if left:   # the names the device leaves to the host, with what it parsed for them
        idx = torch.tensor(left, device=dev)
        noff, nlen = d_noff[idx].cpu().numpy(), d_nlen[idx].cpu().numpy()
        v4, v6 = d_v4.view(n, 4)[idx].cpu().numpy(), d_v6.view(n, 16)[idx].cpu().numpy()
        fl, port = d_fl[idx].cpu().numpy(), d_port[idx].cpu().numpy().view(np.uint16)
        for k, i in enumerate(left):
            name = buf[int(noff[k]):int(noff[k]) + int(nlen[k])].tobytes()
            host[i] = (name, v4[k].tobytes() if fl[k] & HAS_IPV4 else None, v6[k].tobytes() if fl[k] & HAS_IPV6 else None,
                       int(port[k]))
    out = []
    for i in range(n):
        if st[i] != _lib.HYOBFS_OK:
            out.append(None)
        elif i in host:
            name, a, b, port = host[i]
            out.append(rules.decision(rules.match_host(name, a, b, acl.PROTO_UDP, port)))
        else:
            _lib.check(int(res[i]["status"]), "acl_match_batch item")
            out.append(rules.decision(int(res[i]["rule"])))
    return out
