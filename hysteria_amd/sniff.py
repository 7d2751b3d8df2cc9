"""The protocol sniffer: TLS / QUIC server names and HTTP request hosts -- ``extras/sniff/sniff.go`` on MI355X.

==================================================  ==================================================
reference (Go)                                      here
==================================================  ==================================================
``Sniffer{Timeout, RewriteDomain, TCPPorts,         ``Sniffer(timeout, rewrite_domain, tcp_ports,
UDPPorts}`` (sniff.go:31-36)                        udp_ports)``
``(*Sniffer).Check`` (:67-89)                       ``Sniffer.check(is_udp, req_addr)``
``(*Sniffer).UDP`` (:159-174)                       ``Sniffer.udp_many(datagrams, req_addrs)`` and
                                                    ``quic_sniff_batch`` (GPU, many packets)
``(*Sniffer).TCP`` (:91-157)                        ``Sniffer.tcp_many(stream_prefixes, req_addrs)`` and
                                                    ``tcp_sniff_batch`` (GPU)
``(*Sniffer).TCP``, the HTTP branch (:110-127)      ``http_request_host_batch`` (GPU)
``(*Sniffer).TCP``, the TLS branch (:128-144)       ``Sniffer.tls_many(stream_prefixes, req_addrs)`` and
                                                    ``tls_record_sni_batch`` (GPU)
``utls.UnmarshalClientHello(pl).ServerName``        ``client_hello_sni_batch`` (GPU)
``net.SplitHostPort`` / ``net.JoinHostPort``        ``split_host_port`` / ``join_host_port``
==================================================  ==================================================

The parse runs in ``libhyobfs.so`` (``include/hyobfs_sniff.h`` states its rules
and the divergences from the reference's parsers); there is no CPU path.
``Sniffer`` works on whole batches: a caller collects the first datagram (or the
first stream bytes) of many new connections and gets every rewritten request
address back from one call.  Reading from a stream under ``timeout`` is the
caller's; a prefix that does not yet hold the whole record leaves its address
unchanged, as the reference does when its deadline passes.

The HTTP branch answers ``ERR_HOST`` ("left to the host") for the rarer request
forms whose answer the library leaves to the caller's own ``http.ReadRequest``
(an absolute-form or CONNECT target, folded header lines, Transfer-Encoding,
Trailer, an odd Content-Length, a Host value with an empty host part).  This
mirror has no ``net/http``: ``Sniffer.tcp_many`` keeps such an item's address
unchanged, where the reference might rewrite it.
"""
from __future__ import annotations

import ipaddress
import re

import numpy as np

from . import _lib, quic
from ._dev import _pack, _ptr, _records, _stream, _to
from ._lib import _i32, _u32, _u64, _vp

MAX_EXTENSIONS = 256
MAX_NAME_LEN = 255   # a DNS name on the wire; the default name_stride
MAX_HTTP_HEADER_BYTES = 256 * 1024   # sniffMaxHTTPHeaderBytes (sniff.go:21): what the HTTP branch reads of a stream

ERRORS = {
    -54: "not a client hello",
    -55: "malformed client hello",
    -56: "server name larger than the name slot",
    -57: "too many extensions",
    -58: "not a TLS record",
    -59: "record not complete yet",
    -60: "no crypto payload",
    -65: "not an HTTP request",
    -66: "request left to the host's parser",
    -67: "neither HTTP nor TLS",
}
ERR_NOT_HELLO, ERR_MALFORMED, ERR_NAME_CAP, ERR_EXTENSIONS, ERR_NOT_TLS, ERR_NEED_MORE, ERR_NO_PAYLOAD = \
    range(-54, -61, -1)
ERR_NOT_HTTP, ERR_HOST, ERR_UNRECOGNIZED = -65, -66, -67   # -61 .. -64 are the ACL's


class SniffError(ValueError):
    def __init__(self, status: int):
        self.status = status
        super().__init__(f"{ERRORS.get(status, 'error')} ({status})")


# struct hyobfs_sniff_result as a numpy record
SNIFF_RESULT_DTYPE = np.dtype([("status", "<i4"), ("name_len", "<u4"), ("name_off", "<u4"), ("need", "<u4")])
assert SNIFF_RESULT_DTYPE.itemsize == 16


_SIG = {   # include/hyobfs_sniff.h
    "hyobfs_tls_client_hello_sni_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp]),
    "hyobfs_tls_record_sni_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp]),
    "hyobfs_http_request_host_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp]),
    "hyobfs_tcp_sniff_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp]),
    "hyobfs_quic_sniff_workspace_size": (_u64, [_u64]),
    "hyobfs_quic_sniff_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
}


def _slib(lib=None):
    return _lib.declare(quic._qlib(lib), "sniff", _SIG)   # quic_snis also reads quic's results


# ------------------------------------------------------------------ device batches
def client_hello_sni_batch(msgs, off, lens, n: int, names, name_stride: int, res, stream=None) -> None:
    """hyobfs_tls_client_hello_sni_batch: the server name of n device-resident
    ClientHello messages to names[i * name_stride, +name_len); ``res`` gets
    SNIFF_RESULT_DTYPE records.  Arguments are device tensors or pointers."""
    st = _slib().hyobfs_tls_client_hello_sni_batch(_ptr(msgs), _ptr(off), _ptr(lens), n, _ptr(names), name_stride,
                                                   _ptr(res), _stream(stream, res))
    _lib.check(st, "tls_client_hello_sni_batch")


def tls_record_sni_batch(msgs, off, lens, n: int, names, name_stride: int, res, stream=None) -> None:
    """hyobfs_tls_record_sni_batch: the same over the first bytes of n TCP
    streams (isTLS, the record length, then the record's body)."""
    st = _slib().hyobfs_tls_record_sni_batch(_ptr(msgs), _ptr(off), _ptr(lens), n, _ptr(names), name_stride,
                                             _ptr(res), _stream(stream, res))
    _lib.check(st, "tls_record_sni_batch")


def http_request_host_batch(msgs, off, lens, n: int, names, name_stride: int, res, stream=None) -> None:
    """hyobfs_http_request_host_batch: the host part of the Host header of n TCP
    stream prefixes (isHTTP, then rules H0-H7 of include/hyobfs_sniff.h)."""
    st = _slib().hyobfs_http_request_host_batch(_ptr(msgs), _ptr(off), _ptr(lens), n, _ptr(names), name_stride,
                                                _ptr(res), _stream(stream, res))
    _lib.check(st, "http_request_host_batch")


def tcp_sniff_batch(msgs, off, lens, n: int, names, name_stride: int, res, stream=None) -> None:
    """hyobfs_tcp_sniff_batch: Sniffer.TCP's dispatch over n TCP stream prefixes
    in one launch (HTTP, else TLS, else ERR_UNRECOGNIZED)."""
    st = _slib().hyobfs_tcp_sniff_batch(_ptr(msgs), _ptr(off), _ptr(lens), n, _ptr(names), name_stride,
                                        _ptr(res), _stream(stream, res))
    _lib.check(st, "tcp_sniff_batch")


def quic_sniff_workspace_size(n: int) -> int:
    return int(_slib().hyobfs_quic_sniff_workspace_size(n))


def quic_sniff_batch(packets, off, lens, n: int, crypto, crypto_off, crypto_cap, qres, names, name_stride: int,
                     sres, workspace, stream=None) -> None:
    """hyobfs_quic_sniff_batch: read_crypto_payload_batch (in place; ``qres`` and
    ``crypto`` as that call leaves them), then the server name of every payload."""
    st = _slib().hyobfs_quic_sniff_batch(_ptr(packets), _ptr(off), _ptr(lens), n, _ptr(crypto), _ptr(crypto_off),
                                         _ptr(crypto_cap), _ptr(qres), _ptr(names), name_stride, _ptr(sres),
                                         _ptr(workspace), _stream(stream, sres))
    _lib.check(st, "quic_sniff_batch")


def _names(res, host_names, stride):
    """Per record: the name (bytes, b"" for a hello without one) or a SniffError."""
    out = []
    for i, r in enumerate(res):
        if r["status"]:
            out.append(SniffError(int(r["status"])))
        else:
            out.append(host_names[i * stride:i * stride + int(r["name_len"])].tobytes())
    return out


def _sni_many(call, msgs, device, name_stride):
    import torch
    dev = torch.device("cuda", device)
    n = len(msgs)
    if n == 0:
        return []
    buf, off, lens = _pack(msgs)
    d_names = torch.zeros(n * name_stride, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * SNIFF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    call(_to(dev, buf), _to(dev, off), _to(dev, lens), n, d_names, name_stride, d_res)
    return _names(_records(d_res, SNIFF_RESULT_DTYPE), d_names.cpu().numpy(), name_stride)


def client_hello_snis(msgs, device: int = 0, name_stride: int = MAX_NAME_LEN):
    """Server names of a list of ClientHello messages on cuda:<device>: bytes or a SniffError each."""
    return _sni_many(client_hello_sni_batch, msgs, device, name_stride)


def tls_record_snis(prefixes, device: int = 0, name_stride: int = MAX_NAME_LEN):
    """Server names of a list of TCP stream prefixes on cuda:<device>: bytes or a SniffError each."""
    return _sni_many(tls_record_sni_batch, prefixes, device, name_stride)


def http_request_hosts(prefixes, device: int = 0, name_stride: int = MAX_NAME_LEN):
    """Request hosts of a list of TCP stream prefixes on cuda:<device>: bytes or a SniffError each."""
    return _sni_many(http_request_host_batch, prefixes, device, name_stride)


def tcp_snis(prefixes, device: int = 0, name_stride: int = MAX_NAME_LEN):
    """What Sniffer.TCP finds in a list of TCP stream prefixes on cuda:<device>
    (an HTTP request's host or a ClientHello's server name): bytes or a SniffError each."""
    return _sni_many(tcp_sniff_batch, prefixes, device, name_stride)


def quic_snis(packets, device: int = 0, crypto_cap: int = 4096, name_stride: int = MAX_NAME_LEN):
    """Server names of a list of QUIC client Initials on cuda:<device>: bytes or a
    SniffError each (NO_PAYLOAD where ReadCryptoPayload failed).  A payload larger
    than ``crypto_cap`` is read again with the reference's 256 KiB limit."""
    import torch
    dev = torch.device("cuda", device)
    n = len(packets)
    if n == 0:
        return []
    buf, off, lens = _pack(packets)
    d_crypto = torch.zeros(n * crypto_cap, dtype=torch.uint8, device=dev)
    d_qres = torch.zeros(n * quic.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_names = torch.zeros(n * name_stride, dtype=torch.uint8, device=dev)
    d_sres = torch.zeros(n * SNIFF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(quic_sniff_workspace_size(n), 1), dtype=torch.uint8, device=dev)
    quic_sniff_batch(_to(dev, buf), _to(dev, off), _to(dev, lens), n, d_crypto,
                     _to(dev, np.arange(n, dtype=np.uint64) * np.uint64(crypto_cap)),
                     _to(dev, np.full(n, crypto_cap, np.uint32)), d_qres, d_names, name_stride, d_sres, ws)
    out = _names(_records(d_sres, SNIFF_RESULT_DTYPE), d_names.cpu().numpy(), name_stride)
    qres = _records(d_qres, quic.RESULT_DTYPE)
    big = [i for i in range(n) if qres[i]["status"] == quic.ERR_OUT_CAP]
    if big and crypto_cap < quic.MAX_CRYPTO_PAYLOAD_LEN:
        again = quic_snis([packets[i] for i in big], device, max(quic.MAX_CRYPTO_PAYLOAD_LEN,
                                                                 max(len(packets[i]) for i in big)), name_stride)
        for i, r in zip(big, again):
            out[i] = r
    return out


# ------------------------------------------------------------------ addresses (Go's net package)
def split_host_port(hostport: str) -> tuple[str, str]:
    """net.SplitHostPort: ("host", "port") of "host:port", "[host]:port"; ValueError otherwise."""
    i = hostport.rfind(":")
    if i < 0:
        raise ValueError(f"address {hostport}: missing port in address")
    j = k = 0
    if hostport.startswith("["):
        end = hostport.find("]")
        if end < 0:
            raise ValueError(f"address {hostport}: missing ']' in address")
        if end + 1 == len(hostport):
            raise ValueError(f"address {hostport}: missing port in address")
        if end + 1 != i:
            what = "too many colons" if hostport[end + 1] == ":" else "missing port"
            raise ValueError(f"address {hostport}: {what} in address")
        host = hostport[1:end]
        j, k = 1, end + 1
    else:
        host = hostport[:i]
        if ":" in host:
            raise ValueError(f"address {hostport}: too many colons in address")
    if "[" in hostport[j:]:
        raise ValueError(f"address {hostport}: unexpected '[' in address")
    if "]" in hostport[k:]:
        raise ValueError(f"address {hostport}: unexpected ']' in address")
    return host, hostport[i + 1:]


def join_host_port(host: str, port: str) -> str:
    """net.JoinHostPort: brackets around a host that holds ':' or '%'."""
    if ":" in host or "%" in host:
        return f"[{host}]:{port}"
    return f"{host}:{port}"


def _is_ip(host: str) -> bool:
    """net.ParseIP(host) != nil: dotted IPv4 or IPv6 without a zone."""
    try:
        ipaddress.ip_address(host)
    except ValueError:
        return False
    return "%" not in host


class Sniffer:
    """Sniffer (sniff.go:31-36) over batches, on one GPU.  ``tcp_ports`` /
    ``udp_ports``: None for all ports (a nil PortUnion), else (first, last) pairs."""

    def __init__(self, timeout: float = 0.0, rewrite_domain: bool = False, tcp_ports=None, udp_ports=None):
        self.timeout = timeout
        self.rewrite_domain = rewrite_domain
        self.tcp_ports = tcp_ports
        self.udp_ports = udp_ports

    def check(self, is_udp: bool, req_addr: str) -> bool:
        """Check (sniff.go:67-89): whether this request's first bytes get sniffed."""
        if req_addr.startswith("@"):   # internal (e.g. speed test)
            return False
        try:
            host, port = split_host_port(req_addr)
        except ValueError:
            return False
        if not self.rewrite_domain and not _is_ip(host):
            return False
        if not re.fullmatch(r"[+-]?[0-9]+", port):   # strconv.Atoi
            return False
        num = int(port) & 0xFFFF                     # uint16(portNum)
        ports = self.udp_ports if is_udp else self.tcp_ports
        return ports is None or any(lo <= num <= hi for lo, hi in ports)

    @staticmethod
    def _rewrite(req_addr: str, name) -> str:
        if isinstance(name, SniffError) or not name:
            return req_addr
        _, port = split_host_port(req_addr)
        return join_host_port(name.decode("utf-8", "surrogateescape"), port)

    def _many(self, is_udp, snis, items, req_addrs, device):
        if len(items) != len(req_addrs):
            raise ValueError("one request address per item")
        out = list(req_addrs)
        todo = [i for i, a in enumerate(req_addrs) if self.check(is_udp, a)]
        for i, name in zip(todo, snis([items[i] for i in todo], device)):
            out[i] = self._rewrite(req_addrs[i], name)
        return out

    def udp_many(self, datagrams, req_addrs, device: int = 0) -> list[str]:
        """Check, then UDP (sniff.go:159-174), per datagram: the request address,
        rewritten to the QUIC ClientHello's server name where there is one."""
        return self._many(True, quic_snis, datagrams, req_addrs, device)

    def tls_many(self, stream_prefixes, req_addrs, device: int = 0) -> list[str]:
        """Check, then the TLS branch of TCP (sniff.go:128-152), per stream prefix."""
        return self._many(False, tls_record_snis, stream_prefixes, req_addrs, device)

    def tcp_many(self, stream_prefixes, req_addrs, device: int = 0) -> list[str]:
        """Check, then TCP (sniff.go:91-157), per stream prefix: the request address,
        rewritten to an HTTP request's host or a ClientHello's server name where
        there is one.  An item the library leaves to the host (ERR_HOST) keeps its
        address: this mirror has no http.ReadRequest to fall back on."""
        return self._many(False, lambda items, device: tcp_snis(items, device), stream_prefixes, req_addrs, device)
