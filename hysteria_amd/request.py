"""The request hook -- what ``core/server/server.go`` does with a new request
before it dials, on MI355X.

==================================================  ==================================================
reference (Go)                                      here
==================================================  ==================================================
``ReadTCPRequest`` (protocol/proxy.go:39-67)        ``read_tcp_request``, ``tcp_request_parse_batch`` (GPU)
``WriteTCPRequest`` (:69-84)                        ``write_tcp_request``
``ReadTCPResponse`` (:93-129)                       ``read_tcp_response``
``WriteTCPResponse`` (:131-149)                     ``write_tcp_response``, ``tcp_response_build_batch`` (GPU)
``padding.String`` (padding.go:17-24)               ``padding`` (rule G: a stated divergence)
``ParsePortUnion`` (extras/utils/portunion.go)      ``parse_port_union``, ``PortSet`` (GPU)
``Sniffer.Check`` (extras/sniff/sniff.go:67-89)     ``check``, ``sniff_check_batch`` (GPU)
``*reqAddr = net.JoinHostPort(name, port)``         ``rewrite``, ``request_rewrite_batch`` (GPU)
``handleTCPRequest`` up to the dial                 ``tcp_request_decisions``
(server.go:256-335)
the hook in front of a relay datagram's ACL         ``hooked_relay_acl_decisions``
(server.go:405-406)
==================================================  ==================================================

``include/hyobfs_request.h`` states the rules.  Everything runs in
``libhyobfs.so``; there is no Python path.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from ._dev import _pack, _ptr, _records, _stream, _to

FRAME_TYPE, MAX_ADDR, MAX_MSG, MAX_PADDING = 0x401, 2048, 2048, 4096
(ERR_NEED_MORE, ERR_ADDR_LEN, ERR_PADDING_LEN, ERR_MSG_LEN, ERR_CAP, ERR_NO_ADDR, ERR_HOST,
 ERR_UNION) = range(-86, -94, -1)
ERRORS = {
    ERR_NEED_MORE: "the frame is not complete yet",
    ERR_ADDR_LEN: "invalid address length",
    ERR_PADDING_LEN: "invalid padding length",
    ERR_MSG_LEN: "invalid message length",
    ERR_CAP: "the output row is too short",
    ERR_NO_ADDR: "the request has no address",
    ERR_HOST: "left to the host",
    ERR_UNION: "invalid port union",
}
PADDING_CHARS = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
TCP_RESPONSE_PADDING = (128, 1024)   # tcpResponsePadding, [min, max)
TCP_REQUEST_PADDING = (64, 512)      # tcpRequestPadding
MSG_HOOKED, MSG_CONNECTED = b"RequestHook enabled", b"Connected"   # server.go:273, :320

PORT_RANGE_DTYPE = np.dtype([("start", "<u2"), ("end", "<u2")])


class RequestError(ValueError):
    def __init__(self, status: int, need: int = 0):
        self.status, self.need = status, need
        super().__init__(f"{ERRORS.get(status, 'error')} ({status})")


def _rqlib(lib=None):
    return _lib.declare(lib or _lib.load(), "request", _lib._REQ_SIG)


def _buf(b: bytes):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def _bytes(text) -> bytes:
    return text.encode("utf-8", "surrogateescape") if isinstance(text, str) else bytes(text)


def _ranges(ports):
    """(pointer or None, n) of a union: None is the nil union (n = -1)."""
    if ports is None:
        return None, -1, None
    arr = np.array([tuple(r) for r in ports], PORT_RANGE_DTYPE).reshape(-1)
    return (arr.ctypes.data if len(arr) else None), len(arr), arr


# ------------------------------------------------------------------ host, scalar
def tcp_request_record(b) -> tuple[int, int, int, int, int]:
    """hyobfs_tcp_request_parse: (status, need, addr_off, addr_len, consumed)."""
    b = bytes(b)
    c = _buf(b)
    v = [ctypes.c_uint32() for _ in range(4)]
    st = _rqlib().hyobfs_tcp_request_parse(ctypes.addressof(c), len(b), *(ctypes.byref(x) for x in v))
    return (st, *(x.value for x in v))


def read_tcp_request(b) -> tuple[bytes, int]:
    """ReadTCPRequest over the bytes behind the frame type: (address, bytes consumed);
    RequestError (with ``need`` for ERR_NEED_MORE) otherwise."""
    b = bytes(b)
    st, need, ao, al, used = tcp_request_record(b)
    if st != _lib.HYOBFS_OK:
        raise RequestError(st, need)
    return b[ao:ao + al], used


def tcp_response_record(b) -> tuple[int, int, int, int, int, int]:
    """hyobfs_tcp_response_parse: (status, need, ok, msg_off, msg_len, consumed)."""
    b = bytes(b)
    c = _buf(b)
    need, mo, ml, used, ok = (ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(),
                              ctypes.c_uint8())
    st = _rqlib().hyobfs_tcp_response_parse(ctypes.addressof(c), len(b), ctypes.byref(need), ctypes.byref(ok),
                                            ctypes.byref(mo), ctypes.byref(ml), ctypes.byref(used))
    return st, need.value, ok.value, mo.value, ml.value, used.value


def read_tcp_response(b) -> tuple[bool, bytes, int]:
    """ReadTCPResponse: (ok, message, bytes consumed); RequestError otherwise."""
    b = bytes(b)
    st, need, ok, mo, ml, used = tcp_response_record(b)
    if st != _lib.HYOBFS_OK:
        raise RequestError(st, need)
    return bool(ok), b[mo:mo + ml], used


def _build(fn, head, text, pad_len, seed, item, cap):
    text = _bytes(text)
    cap = len(text) + pad_len + 32 if cap is None else cap
    t, out = _buf(text), (ctypes.c_uint8 * max(cap, 1))()
    n = fn(*head, ctypes.addressof(t), len(text), pad_len, seed, item, ctypes.addressof(out), cap)
    return -1 if n < 0 else bytes(out[:n])


def write_tcp_request(addr, pad_len: int, seed: int = 0, item: int = 0, cap=None):
    """WriteTCPRequest with ``pad_len`` bytes of rule G's padding: the frame, or -1 when ``cap`` is too small."""
    return _build(_rqlib().hyobfs_tcp_request_build, (), addr, pad_len, seed, item, cap)


def write_tcp_response(ok: bool, msg, pad_len: int, seed: int = 0, item: int = 0, cap=None):
    """WriteTCPResponse with ``pad_len`` bytes of rule G's padding: the frame, or -1 when ``cap`` is too small."""
    return _build(_rqlib().hyobfs_tcp_response_build, (1 if ok else 0,), msg, pad_len, seed, item, cap)


def padding(seed: int, item: int, length: int) -> bytes:
    """hyobfs_req_padding_fill: rule G's bytes for (seed, item)."""
    out = (ctypes.c_uint8 * max(length, 1))()
    _rqlib().hyobfs_req_padding_fill(seed, item, ctypes.addressof(out), length)
    return bytes(out[:length])


def parse_port_union(text):
    """ParsePortUnion: the normalised [(start, end)], or None where the reference returns nil."""
    t = _bytes(text)
    b, n = _buf(t), ctypes.c_uint32()
    cap = len(t) // 2 + 2
    out = np.zeros(cap, PORT_RANGE_DTYPE)
    st = _rqlib().hyobfs_port_union_parse(ctypes.addressof(b), len(t), out.ctypes.data, cap, ctypes.byref(n))
    if st == ERR_UNION:
        return None
    _lib.check(st, "port_union_parse")
    return [(int(r["start"]), int(r["end"])) for r in out[:n.value]]


def port_union_contains(ports, port: int) -> bool:
    """PortUnion.Contains; ``ports`` None is the nil union (every port)."""
    p, n, _keep = _ranges(ports)
    return _rqlib().hyobfs_port_union_contains(p, n, port) == 1


def check(text, is_udp: bool, rewrite_domain: bool = False, tcp_ports=None, udp_ports=None) -> bool:
    """Sniffer.Check (hyobfs_sniff_check): unions are [(start, end)] or None for nil."""
    t = _bytes(text)
    b = _buf(t)
    tp, tn, _k1 = _ranges(tcp_ports)
    up, un, _k2 = _ranges(udp_ports)
    return _rqlib().hyobfs_sniff_check(ctypes.addressof(b), len(t), int(is_udp), int(rewrite_domain), tp, tn, up, un) == 1


def rewrite(addr, checked: bool, name=b"", sniff_status: int = 0, cap=None):
    """hyobfs_request_rewrite: (address text, rewritten); -1 for a ``cap`` that is too
    small; RequestError(ERR_HOST) where the item is left to the host."""
    a, nm = _bytes(addr), _bytes(name)
    cap = len(a) + len(nm) + 3 if cap is None else cap
    ab, nb, out, rew = _buf(a), _buf(nm), (ctypes.c_uint8 * max(cap, 1))(), ctypes.c_uint8()
    n = _rqlib().hyobfs_request_rewrite(ctypes.addressof(ab), len(a), int(checked), ctypes.addressof(nb), len(nm),
                                        sniff_status, ctypes.addressof(out), cap, ctypes.byref(rew))
    if n == -1:
        return -1
    if n < 0:
        raise RequestError(int(n))
    return bytes(out[:n]), bool(rew.value)


# ------------------------------------------------------------------ device
class PortSet:
    """hyobfs_portset: a port union as a 65536-bit map on cuda:<device>.  ``ports``
    is [(start, end)] in any order; ``PortSet.of(None, ...)`` is None, the nil union."""

    def __init__(self, ports, device: int = 0):
        p, n, _keep = _ranges(list(ports))
        h = ctypes.c_void_p()
        _lib.check(_rqlib().hyobfs_portset_new(p, n, device, ctypes.byref(h)), "portset_new")
        self.handle, self.device = h, device

    @classmethod
    def of(cls, ports, device: int = 0):
        return None if ports is None else cls(ports, device)

    def close(self):
        h, self.handle = self.handle, None
        if h:
            _rqlib().hyobfs_portset_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


def _handle(portset):
    return portset.handle if isinstance(portset, PortSet) else portset


def tcp_request_parse_batch(src, off, len_, n: int, status, need, addr_off, addr_len, rest_off, rest_len,
                            stream=None) -> None:
    """hyobfs_tcp_request_parse_batch: rule R over the stream prefixes src[off[i], +len_[i])."""
    st = _rqlib().hyobfs_tcp_request_parse_batch(_ptr(src), _ptr(off), _ptr(len_), n, _ptr(status), _ptr(need),
                                                 _ptr(addr_off), _ptr(addr_len), _ptr(rest_off), _ptr(rest_len),
                                                 _stream(stream, status))
    _lib.check(st, "tcp_request_parse_batch")


def sniff_check_batch(src, off, len_, status_in, n: int, is_udp: bool, rewrite_domain: bool, portset, check_out,
                      stream=None) -> None:
    """hyobfs_sniff_check_batch: rule C over the texts src[off[i], +len_[i]); ``portset`` is a PortSet or None."""
    st = _rqlib().hyobfs_sniff_check_batch(_ptr(src), _ptr(off), _ptr(len_), _ptr(status_in), n, int(is_udp),
                                           int(rewrite_domain), _handle(portset), _ptr(check_out),
                                           _stream(stream, check_out))
    _lib.check(st, "sniff_check_batch")


def request_rewrite_batch(src, off, len_, status_in, check_in, names, name_stride: int, sres, n: int, out,
                          out_stride: int, base_off: int, row_off, out_len, rewritten, status, stream=None) -> None:
    """hyobfs_request_rewrite_batch: rule W; ``out``, ``row_off`` and ``out_len`` then feed ``addr.parse_batch``."""
    st = _rqlib().hyobfs_request_rewrite_batch(_ptr(src), _ptr(off), _ptr(len_), _ptr(status_in), _ptr(check_in),
                                               _ptr(names), name_stride, _ptr(sres), n, _ptr(out), out_stride, base_off,
                                               _ptr(row_off), _ptr(out_len), _ptr(rewritten), _ptr(status),
                                               _stream(stream, status))
    _lib.check(st, "request_rewrite_batch")


def tcp_response_build_batch(ok, msg_idx, msgs, msg_off, msg_len, n_msgs: int, pad_len, seed: int, n: int, out,
                             out_stride: int, out_len, status, stream=None) -> None:
    """hyobfs_tcp_response_build_batch: rule S; row i is out[i * out_stride, +out_len[i])."""
    st = _rqlib().hyobfs_tcp_response_build_batch(_ptr(ok), _ptr(msg_idx), _ptr(msgs), _ptr(msg_off), _ptr(msg_len),
                                                  n_msgs, _ptr(pad_len), seed, n, _ptr(out), out_stride, _ptr(out_len),
                                                  _ptr(status), _stream(stream, status))
    _lib.check(st, "tcp_response_build_batch")


# ------------------------------------------------------------------ the pipelines, worked
TcpDecisions = namedtuple("TcpDecisions", "status need check decisions addrs responses")
TcpDecisions.__doc__ = """What ``tcp_request_decisions`` returns, per stream:
status (request parse, then rewrite, then address parse: the first that is not 0), need (for ERR_NEED_MORE),
check, decisions ((outbound, hijack) or None), addrs (the address to dial, bytes or None) and responses
(the response frame, bytes or None)."""


def _finish_on_host(rules, proto, left, d_buf, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port, n):
    """The names the ACL leaves to the host (ERR_HOST), with what the device parsed for them."""
    import torch

    from . import addr
    if not left:
        return {}
    idx = torch.tensor(left, device=d_buf.device)
    noff, nlen = d_noff[idx].cpu().numpy(), d_nlen[idx].cpu().numpy()
    v4, v6 = d_v4.view(n, 4)[idx].cpu().numpy(), d_v6.view(n, 16)[idx].cpu().numpy()
    fl, port = d_fl[idx].cpu().numpy(), d_port[idx].cpu().numpy().view(np.uint16)
    out = {}
    for k, i in enumerate(left):
        name = d_buf[int(noff[k]):int(noff[k]) + int(nlen[k])].cpu().numpy().tobytes()
        out[i] = rules.decision(rules.match_host(name, v4[k].tobytes() if fl[k] & addr.HAS_IPV4 else None,
                                                 v6[k].tobytes() if fl[k] & addr.HAS_IPV6 else None, proto,
                                                 int(port[k])))
    return out


def tcp_request_decisions(rules, sniffer, stream_prefixes, device: int = 0, refusals=None, pad_lens=None, seed: int = 0,
                          out_stride: int = 512, name_stride: int = 255, resp_stride: int = 1280):
    """handleTCPRequest up to the dial, worked, for a list of stream prefixes (the
    bytes behind the 0x401 frame type) on one stream of cuda:<device>:
    request parse -> Check -> ``tcp_sniff_batch`` over the bytes behind the request
    -> rewrite -> ``addr.parse_batch`` over the rows -> ``RuleSet.match_batch`` ->
    response rows.  ``sniffer`` is a ``sniff.Sniffer`` (its rewrite_domain and
    tcp_ports are used).  The response says "RequestHook enabled" where Check
    holds (server.go:273), else the text ``refusals`` (outbound -> message) has for
    the decided outbound, with ok = false, else "Connected"; ``pad_lens`` are the
    caller's draw of padding lengths (default: tcpResponsePadding's range, numpy's
    generator seeded with ``seed``).  Only statuses, decisions and the results
    themselves come back; a stream the sniffer leaves to the host (ERR_HOST) gets
    no decision here, and a name the ACL leaves to the host is finished by
    ``match_host``.  An address longer than ``out_stride`` is ERR_CAP."""
    import torch

    from . import acl, addr, sniff
    n = len(stream_prefixes)
    if n == 0:
        return TcpDecisions(np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint8), [], [], [])
    dev = torch.device("cuda", device)
    stream = torch.cuda.current_stream(dev)
    refusals = dict(refusals or {})
    texts = [MSG_HOOKED, MSG_CONNECTED] + [_bytes(t) for t in refusals.values()]
    lut = np.ones(max(list(refusals) + [0]) + 2, np.int32)   # outbound -> message; the last entry: any other outbound
    for k, ob in enumerate(refusals):
        lut[ob] = 2 + k
    if pad_lens is None:
        pad_lens = np.random.default_rng(seed).integers(*TCP_RESPONSE_PADDING, size=n)
    buf, off, lens = _pack(stream_prefixes)
    mbuf, moff, mlen = _pack(texts)
    d_in, d_off, d_len = _to(dev, buf), _to(dev, off), _to(dev, lens)
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda: torch.zeros(n, dtype=torch.int64, device=dev)   # noqa: E731
    u8 = lambda k=n: torch.zeros(k, dtype=torch.uint8, device=dev)   # noqa: E731
    d_st, d_need, d_aoff, d_alen, d_roff, d_rlen = i32(), i32(), i64(), i32(), i64(), i32()
    d_chk, d_names, d_sres = u8(), u8(n * name_stride), u8(n * sniff.SNIFF_RESULT_DTYPE.itemsize)
    d_rows, d_rowoff, d_outlen, d_rew, d_rst = u8(n * out_stride), i64(), i32(), u8(), i32()
    d_res = u8(n * acl.ACL_RESULT_DTYPE.itemsize)
    d_resp, d_resplen, d_respst = u8(n * resp_stride), i32(), i32()
    ports = PortSet.of(sniffer.tcp_ports, device)
    try:
        tcp_request_parse_batch(d_in, d_off, d_len, n, d_st, d_need, d_aoff, d_alen, d_roff, d_rlen, stream=stream)
        sniff_check_batch(d_in, d_aoff, d_alen, d_st, n, False, sniffer.rewrite_domain, ports, d_chk, stream=stream)
        sniff.tcp_sniff_batch(d_in, d_roff, d_rlen, n, d_names, name_stride, d_sres, stream=stream)
        request_rewrite_batch(d_in, d_aoff, d_alen, d_st, d_chk, d_names, name_stride, d_sres, n, d_rows, out_stride, 0,
                              d_rowoff, d_outlen, d_rew, d_rst, stream=stream)
        d_plen = torch.where(d_rst == 0, d_outlen, torch.zeros_like(d_outlen))   # a row that was not written is not read
        d_pst, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port = addr.parse_outputs(n, dev)
        addr.parse_batch(d_rows, d_rowoff, d_plen, n, d_pst, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port, stream=stream)
        d_proto = torch.full((n,), acl.PROTO_TCP, dtype=torch.uint8, device=dev)
        rules.match_batch(d_rows, d_noff, d_nlen, d_v4, d_v6, d_fl, d_proto, d_port, n, d_res, stream=stream,
                          device=device)
        # the response's message: Check's own, else what the decided outbound says
        d_ob = d_res.view(torch.int32).view(n, 4)[:, 2].to(torch.int64)
        d_lut = _to(dev, lut)
        d_midx = torch.where(d_chk != 0, torch.zeros_like(d_st), d_lut[torch.clamp(d_ob, max=len(lut) - 1)])
        d_ok = (d_midx < 2).to(torch.uint8)
        tcp_response_build_batch(d_ok, d_midx, _to(dev, mbuf), _to(dev, moff), _to(dev, mlen), len(texts),
                                 _to(dev, np.asarray(pad_lens, np.uint32).view(np.int32)), seed, n, d_resp, resp_stride,
                                 d_resplen, d_respst, stream=stream)
        st, rst, pst = d_st.cpu().numpy(), d_rst.cpu().numpy(), d_pst.cpu().numpy()
    finally:
        if ports is not None:
            ports.close()
    status = np.where(st != 0, st, np.where(rst != 0, rst, pst)).astype(np.int32)
    res = _records(d_res, acl.ACL_RESULT_DTYPE)
    left = [i for i in range(n) if status[i] == 0 and res[i]["status"] == acl.ERR_HOST]
    host = _finish_on_host(rules, acl.PROTO_TCP, left, d_rows, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port, n)
    rows, outlen = d_rows.cpu().numpy(), d_outlen.cpu().numpy()
    resp, resplen, respst = d_resp.cpu().numpy(), d_resplen.cpu().numpy(), d_respst.cpu().numpy()
    chk = d_chk.cpu().numpy()
    decisions, addrs, responses = [], [], []
    for i in range(n):
        if status[i] != 0:
            decisions.append(None)
            addrs.append(None)
            responses.append(None)
            continue
        addrs.append(rows[i * out_stride:i * out_stride + int(outlen[i])].tobytes())
        if i in host:   # the device could not decide the outbound: the response is the host's as well
            decisions.append(host[i])
            ob = host[i][0]
            msg = MSG_HOOKED if chk[i] else _bytes(refusals[ob]) if ob in refusals else MSG_CONNECTED
            responses.append(write_tcp_response(bool(chk[i]) or ob not in refusals, msg, int(pad_lens[i]), seed, i))
            continue
        _lib.check(int(res[i]["status"]), "acl_match_batch item")
        decisions.append(rules.decision(int(res[i]["rule"])))
        _lib.check(int(respst[i]), "tcp_response_build_batch item")
        responses.append(resp[i * resp_stride:i * resp_stride + int(resplen[i])].tobytes())
    return TcpDecisions(status, d_need.cpu().numpy().view(np.uint32), chk, decisions, addrs, responses)


def hooked_relay_acl_decisions(rules, sniffer, datagrams, device: int = 0, crypto_cap: int = 4096,
                               out_stride: int = 512, name_stride: int = 255):
    """``addr.relay_acl_decisions`` with the request hook in front of the address
    parse (server.go:405-406): ``udpmsg.parse_batch``, Check on each message's
    address, ``quic_sniff_batch`` on its data, the rewrite, ``addr.parse_batch``
    over the rows and ``RuleSet.match_batch``, on one stream.  The address offsets
    and the gate are formed from the parsed records with torch ops on the device.
    Returns per datagram (outbound, hijack address or None), or None where the
    message or its address is refused."""
    import torch

    from . import acl, addr, quic, sniff, udpmsg
    n = len(datagrams)
    if n == 0:
        return []
    dev = torch.device("cuda", device)
    stream = torch.cuda.current_stream(dev)
    buf, off, lens = _pack(datagrams)
    d_in, d_off, d_len = _to(dev, buf), _to(dev, off), _to(dev, lens)
    d_parsed = torch.zeros(n * udpmsg.PARSED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    udpmsg.parse_batch(d_in, d_off, d_len, n, d_parsed, stream=stream)
    rec = d_parsed.view(torch.int32).view(n, 8)   # status, session, ids, addr_off, addr_len, data_off, data_len, -
    d_off64 = d_off.view(torch.int64)
    d_gate = rec[:, 0].contiguous()
    d_aoff, d_alen = (d_off64 + rec[:, 3]).contiguous(), rec[:, 4].contiguous()
    d_doff, d_dlen = (d_off64 + rec[:, 5]).contiguous(), rec[:, 6].contiguous()
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)   # noqa: E731
    u8 = lambda k=n: torch.zeros(k, dtype=torch.uint8, device=dev)   # noqa: E731
    d_chk, d_names, d_sres = u8(), u8(n * name_stride), u8(n * sniff.SNIFF_RESULT_DTYPE.itemsize)
    d_rows, d_rowoff, d_outlen, d_rew, d_rst = (u8(n * out_stride), torch.zeros(n, dtype=torch.int64, device=dev), i32(),
                                                u8(), i32())
    d_res = u8(n * acl.ACL_RESULT_DTYPE.itemsize)
    d_crypto, d_qres = u8(n * crypto_cap), u8(n * quic.RESULT_DTYPE.itemsize)
    ws = torch.empty(max(sniff.quic_sniff_workspace_size(n), 1), dtype=torch.uint8, device=dev)
    ports = PortSet.of(sniffer.udp_ports, device)
    try:
        sniff_check_batch(d_in, d_aoff, d_alen, d_gate, n, True, sniffer.rewrite_domain, ports, d_chk, stream=stream)
        d_pkts = d_in.clone()   # the sniffer unprotects its packets in place
        sniff.quic_sniff_batch(d_pkts, d_doff, d_dlen, n, d_crypto,
                               _to(dev, np.arange(n, dtype=np.uint64) * np.uint64(crypto_cap)),
                               _to(dev, np.full(n, crypto_cap, np.uint32)), d_qres, d_names, name_stride, d_sres, ws,
                               stream=stream)
        request_rewrite_batch(d_in, d_aoff, d_alen, d_gate, d_chk, d_names, name_stride, d_sres, n, d_rows, out_stride,
                              0, d_rowoff, d_outlen, d_rew, d_rst, stream=stream)
        d_plen = torch.where(d_rst == 0, d_outlen, torch.zeros_like(d_outlen))
        d_pst, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port = addr.parse_outputs(n, dev)
        addr.parse_batch(d_rows, d_rowoff, d_plen, n, d_pst, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port, stream=stream)
        d_proto = torch.full((n,), acl.PROTO_UDP, dtype=torch.uint8, device=dev)
        rules.match_batch(d_rows, d_noff, d_nlen, d_v4, d_v6, d_fl, d_proto, d_port, n, d_res, stream=stream,
                          device=device)
        rst, pst = d_rst.cpu().numpy(), d_pst.cpu().numpy()
    finally:
        if ports is not None:
            ports.close()
    res = _records(d_res, acl.ACL_RESULT_DTYPE)
    good = [rst[i] == 0 and pst[i] == 0 for i in range(n)]
    left = [i for i in range(n) if good[i] and res[i]["status"] == acl.ERR_HOST]
    host = _finish_on_host(rules, acl.PROTO_UDP, left, d_rows, d_noff, d_nlen, d_v4, d_v6, d_fl, d_port, n)
    out = []
    for i in range(n):
        if not good[i]:
            out.append(None)
        elif i in host:
            out.append(host[i])
        else:
            _lib.check(int(res[i]["status"]), "acl_match_batch item")
            out.append(rules.decision(int(res[i]["rule"])))
    return out
