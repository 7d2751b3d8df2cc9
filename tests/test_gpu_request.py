"""The request-hook kernels on the GPU (hysteria_amd/csrc/request.hip,
include/hyobfs_request.h): the lattices of tests/request_cases.py through the four
device calls, bit-exact against the restatement (tests/request_ref.py), every output
array between guard bytes and every input in poisoned surroundings; the port set;
and the two worked pipelines against the restated chain."""
import numpy as np
import pytest

import addr_cases as ac
import addr_ref as A
import http_cases as hc
import http_ref
import request_cases as rc
import request_ref as R
import sni_ref
import sniff_cases as sc
import udpmsg_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = rc.GUARD_BYTES   # guard bytes (0xA5) on both sides of every output array


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)   # a writable copy


def _bytes(dev, b: bytes):
    return _t(dev, np.frombuffer(bytes(b) or b"\0", np.uint8))


class Guarded:
    """nbytes of device memory between two runs of PAD guard bytes, all pre-filled with the guard byte; the
    payload starts `mis` bytes past a 16-byte boundary."""

    def __init__(self, dev, nbytes, mis=0):
        self.lead, self.nbytes = PAD + mis, nbytes   # torch allocations are at least 256-aligned
        self.t = torch.full((self.lead + nbytes + PAD,), rc.GUARD, dtype=torch.uint8, device=dev)
        assert self.t.data_ptr() % 16 == 0 and PAD % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead

    def read(self, dtype=np.uint8):
        """The payload, after checking that both guards are intact."""
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == rc.GUARD).all() and (h[self.lead + self.nbytes:] == rc.GUARD).all(), "guard bytes"
        return np.frombuffer(h[self.lead:self.lead + self.nbytes].tobytes(), dtype)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _lib():
    from hysteria_amd import request
    return request._rqlib()


def _ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------ the lattices
@pytest.mark.parametrize("case", rc.parse_cases(), ids=_ids(rc.parse_cases()))
def test_request_parse_lattice(dev, case):
    buf, off, lens = rc.layout(case["items"])
    n = len(off)
    d_buf, d_off, d_len = _bytes(dev, buf), _t(dev, np.array(off, np.uint64)), _t(dev, np.array(lens, np.uint32))
    out = {k: Guarded(dev, n * np.dtype(dt).itemsize) for k, dt in rc.PARSE_OUT}
    rc_ = _lib().hyobfs_tcp_request_parse_batch(d_buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                                *(out[k].ptr for k, _ in rc.PARSE_OUT), _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc_ == 0
    rc.check_parse(case["name"], case["items"], off, {k: out[k].read(dt) for k, dt in rc.PARSE_OUT})


@pytest.mark.parametrize("case", rc.check_cases(), ids=_ids(rc.check_cases()))
def test_check_lattice(dev, case):
    from hysteria_amd import request
    buf, off, lens = rc.layout(case["items"], skip=rc.closed(case))
    n = len(off)
    d_buf, d_off, d_len = _bytes(dev, buf), _t(dev, np.array(off, np.uint64)), _t(dev, np.array(lens, np.uint32))
    d_gate = _t(dev, np.array(rc.gates(case), np.int32)) if case["gate"] else None
    check = Guarded(dev, n)
    ports = request.PortSet.of(case["union"])
    try:
        rc_ = _lib().hyobfs_sniff_check_batch(d_buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                              d_gate.data_ptr() if case["gate"] else None, n, int(case["is_udp"]),
                                              int(case["rewrite_domain"]), ports.handle if ports else None, check.ptr,
                                              _stream(dev))
        torch.cuda.synchronize(dev)
    finally:
        if ports:
            ports.close()
    assert rc_ == 0
    rc.verify_check(case, check.read())


@pytest.mark.parametrize("case", rc.rewrite_cases(), ids=_ids(rc.rewrite_cases()))
def test_rewrite_lattice(dev, case):
    src, off, lens, gate, chk, sres, names = rc.rewrite_inputs(case)
    n, stride = len(off), case["stride"]
    d = [_bytes(dev, src), _t(dev, np.array(off, np.uint64)), _t(dev, np.array(lens, np.uint32)),
         _t(dev, np.array(gate, np.int32)), _t(dev, np.array(chk, np.uint8)), _bytes(dev, names.tobytes()),
         _bytes(dev, sres.tobytes())]
    status, out_len, rew, row_off = Guarded(dev, 4 * n), Guarded(dev, 4 * n), Guarded(dev, n), Guarded(dev, 8 * n)
    out = Guarded(dev, n * stride, case["mis"])
    rc_ = _lib().hyobfs_request_rewrite_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                              d[3].data_ptr() if case["gate"] else None, d[4].data_ptr(), d[5].data_ptr(),
                                              rc.NAME_STRIDE, d[6].data_ptr(), n, out.ptr, stride, rc.BASE_OFF, row_off.ptr,
                                              out_len.ptr, rew.ptr, status.ptr, _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc_ == 0
    rc.verify_rewrite(case, status.read(np.int32), out_len.read(np.uint32), rew.read(), row_off.read(np.uint64), out.read())


@pytest.mark.parametrize("case", rc.response_cases(), ids=_ids(rc.response_cases()))
def test_response_build_lattice(dev, case):
    from hysteria_amd import request
    ok, idx, pad, mbuf, moff, mlen = rc.response_inputs(case)
    n, stride = len(ok), case["stride"]
    d = [_t(dev, ok), _t(dev, idx.view(np.int32)), _bytes(dev, mbuf), _t(dev, moff), _t(dev, mlen.view(np.int32)),
         _t(dev, pad.view(np.int32))]
    status, out_len, out = Guarded(dev, 4 * n), Guarded(dev, 4 * n), Guarded(dev, n * stride, case["mis"])
    rc_ = _lib().hyobfs_tcp_response_build_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                 d[4].data_ptr(), len(rc.MSGS), d[5].data_ptr(), rc.SEED, n, out.ptr, stride,
                                                 out_len.ptr, status.ptr, _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc_ == 0
    rc.verify_response(case, status.read(np.int32), out_len.read(np.uint32), out.read(),
                       parse_back=request.tcp_response_record)


def test_port_set_is_rule_k(dev):
    """Every port of every union, one text each: the bit map says what Contains says, ranges in any order."""
    from hysteria_amd import request
    ports = [0, 1, 69, 70, 79, 80, 81, 85, 86, 89, 90, 100, 101, 442, 443, 444, 65534, 65535]
    items = [b"1.2.3.4:%d" % p for p in ports]
    buf, off, lens = rc.layout(items)
    d_buf, d_off, d_len = _bytes(dev, buf), _t(dev, np.array(off, np.uint64)), _t(dev, np.array(lens, np.uint32))
    for u in rc.UNIONS + [[(65535, 65535), (0, 0)], [(0, 65535)], [(100, 65535), (0, 79)]]:
        check = torch.full((len(items),), 7, dtype=torch.uint8, device=dev)
        with (request.PortSet(u) if u is not None else _Null()) as ps:
            request.sniff_check_batch(d_buf, d_off, d_len, None, len(items), False, False, ps, check)
            torch.cuda.synchronize(dev)
        assert [int(x) for x in check.cpu()] == [int(R.contains(u, p)) for p in ports], u


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def test_refusals_run_no_kernel(dev):
    from hysteria_amd import _lib as L
    lib, N = _lib(), None
    g = Guarded(dev, 256)
    p, s = g.ptr, _stream(dev)
    parse = [p, p, p, 1, p, p, p, p, p, p, s]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        a = list(parse)
        a[k] = N
        assert lib.hyobfs_tcp_request_parse_batch(*a) == L.HYOBFS_ERR_INVALID
    check = [p, p, p, N, 1, 0, 0, N, p, s]
    for k in (0, 1, 2, 8):
        a = list(check)
        a[k] = N
        assert lib.hyobfs_sniff_check_batch(*a) == L.HYOBFS_ERR_INVALID
    check[5] = 2
    assert lib.hyobfs_sniff_check_batch(*check) == L.HYOBFS_ERR_INVALID
    rew = [p, p, p, N, p, p, 16, p, 1, p, 64, 0, p, p, p, p, s]
    for k in (0, 1, 2, 4, 5, 7, 9, 12, 13, 14, 15):
        a = list(rew)
        a[k] = N
        assert lib.hyobfs_request_rewrite_batch(*a) == L.HYOBFS_ERR_INVALID
    rew[10] = 0
    assert lib.hyobfs_request_rewrite_batch(*rew) == L.HYOBFS_ERR_INVALID
    resp = [p, p, p, p, p, 1, p, 0, 1, p, 64, p, p, s]
    for k in (0, 1, 2, 3, 4, 6, 9, 11, 12):
        a = list(resp)
        a[k] = N
        assert lib.hyobfs_tcp_response_build_batch(*a) == L.HYOBFS_ERR_INVALID
    torch.cuda.synchronize(dev)
    assert (g.read() == rc.GUARD).all()   # nothing ran


# ------------------------------------------------------------------ the pipelines
RULES = """
pinned(1.2.3.4)
lan(10.0.0.0/8)
site(suffix:example.com, *, 9.9.9.9)
reject(suffix:bad.test)
idn(政府.中国)
games(all, udp/1000-2000)
web(all, tcp/8080)
"""
OUTBOUNDS = {"pinned": 1, "lan": 2, "site": 3, "reject": 4, "idn": 5, "games": 6, "web": 7}
REFUSALS = {4: "connection rejected by the ACL", 2: b"no route to the LAN"}


def _hello(name: bytes) -> bytes:
    return sc.with_sni(sc.sni_body([(0, name)]))


def tcp_streams():
    tls = sc.as_record(_hello(b"www.example.com"))
    http = hc.req(headers=(b"Host: x.bad.test:8080", b"Accept: */*"))
    payloads = [tls, http, hc.req(headers=(b"Host: [2001:db8::1]:80",)), tls[:40], b"", b"\x00\x01\x02\x03 not a protocol",
                hc.req(line=b"GET http://other.org/ HTTP/1.1"), hc.req(headers=(b"Accept: */*",)),
                sc.as_record(_hello("政府.中国".encode())), sc.as_record(_hello(b"1.2.3.4")), http[:20]]
    addrs = [b"1.2.3.4:443", b"10.1.2.3:+8080", b"www.example.com:443", b"[2001:db8::1]:80", b"11.0.0.1:65616", b"@SpeedTest",
             b"9.9.9.9:-1", b"nocolon", b"8.8.8.8:x", b"x.bad.test:80", b"10.9.9.9:81"]
    out = [rc.request(a, 1 + 7 * k % 90, p) for k, (a, p) in enumerate((a, p) for a in addrs for p in payloads)]
    out += [b"", b"\x05a:1", rc.request(b"", 0, tls), R.varint(2049, 2) + b"x" * 2049, rc.request(b"1.2.3.4:80", 4097, tls),
            rc.request(b"1.2.3.4:80", 50, tls)[:30], rc.request(ac._host(600) + b":80", 3, tls), rc.request(ac._host(600) + b":81", 3, tls)]
    return out


def expected_tcp(rs, sniffer, streams, pad_lens, seed, out_stride=512):
    from hysteria_amd import acl
    status, checks, decisions, addrs, responses = [], [], [], [], []
    for i, p in enumerate(streams):
        st, need, ao, al, used = R.read_tcp_request(p)
        chk, text = 0, None
        if st == R.OK:
            addr, rest = p[ao:ao + al], p[used:]
            chk = int(R.check(addr, False, sniffer.rewrite_domain, sniffer.tcp_ports, sniffer.udp_ports))
            sst, nlen, noff, _, name = http_ref.tcp_sniff(rest)
            st, text, _ = R.rewrite(addr, bool(chk), name, sst)
            if st == R.OK and len(text) > out_stride:
                st = R.CAP
        if st == R.OK:
            st, no, nl, v4, v6, fl, port = A.parse(text)
        status.append(st)
        checks.append(chk)
        if st != R.OK:
            decisions.append(None)
            addrs.append(None)
            responses.append(None)
            continue
        d = rs.decision(rs.match_host(text[no:no + nl], v4 if fl & 1 else None, v6 if fl & 2 else None, acl.PROTO_TCP, port))
        decisions.append(d)
        addrs.append(text)
        msg = b"RequestHook enabled" if chk else REFUSALS.get(d[0], b"Connected")
        msg = msg.encode() if isinstance(msg, str) else msg
        responses.append(R.write_tcp_response(bool(chk) or d[0] not in REFUSALS, msg, int(pad_lens[i]), seed, i))
    return status, checks, decisions, addrs, responses


@pytest.mark.parametrize("rewrite_domain,tcp_ports", [(False, None), (True, [(443, 443), (80, 80), (8080, 8080)])])
def test_tcp_request_decisions(dev, rewrite_domain, tcp_ports):
    import hysteria_amd
    streams = tcp_streams()
    sniffer = hysteria_amd.Sniffer(rewrite_domain=rewrite_domain, tcp_ports=tcp_ports)
    pad_lens = [128 + (37 * i) % 896 for i in range(len(streams))]
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(RULES), OUTBOUNDS) as rs:
        got = hysteria_amd.tcp_request_decisions(rs, sniffer, streams, refusals=REFUSALS, pad_lens=pad_lens, seed=77)
        status, checks, decisions, addrs, responses = expected_tcp(rs, sniffer, streams, pad_lens, 77)
        empty = hysteria_amd.tcp_request_decisions(rs, sniffer, [])
    assert [int(x) for x in got.status] == status
    assert [int(x) for x in got.check] == checks
    assert got.addrs == addrs and got.decisions == decisions and got.responses == responses
    assert len(empty.status) == 0 and empty.decisions == []
    # the lattice is not vacuous: every branch of the chain is taken
    assert {R.OK, R.NEED_MORE, R.ADDR_LEN, R.PADDING_LEN, R.HOST, R.CAP, A.MISSING_PORT, A.PORT} <= set(status)
    assert 0 < sum(checks) < len(checks) and sum(a is not None and b"example.com" in a for a in addrs) >= 1
    assert addrs[0] == b"www.example.com:443" and decisions[0] == (3, "9.9.9.9")   # 1.2.3.4:443 with a TLS hello
    assert {True, False} <= {R.read_tcp_response(r)[2] == 1 for r in responses if r is not None}


def relay_datagrams():
    hellos = [_hello(b"www.example.com"), _hello(b"x.bad.test"), sc.hello([]), _hello(b"fe80::1")]
    addrs = [b"1.2.3.4:443", b"10.1.2.3:1500", b"other.org:1500", b"[2001:db8::1]:+443", b"11.0.0.1:65979", b"9.9.9.9:x", b"nocolon"]
    out = []
    for k, (a, h) in enumerate((a, h) for a in addrs for h in range(len(hellos) + 2)):
        data = sc.initial_for(hellos[h], k) if h < len(hellos) else (b"not quic at all" if h == len(hellos) else b"\xc3" * 30)
        out.append(ac.datagram(a, data=data, session=k + 1))
    out.insert(2, bytes(5))
    out.insert(11, ac.datagram(b"a:1", data=b""))
    return out


def test_hooked_relay_acl_decisions(dev):
    import hysteria_amd
    import quic_cases as qc
    from hysteria_amd import acl
    ds = relay_datagrams()
    for rewrite_domain, udp_ports in ((False, None), (True, [(443, 443), (1000, 2000)])):
        sniffer = hysteria_amd.Sniffer(rewrite_domain=rewrite_domain, udp_ports=udp_ports)
        with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(RULES), OUTBOUNDS) as rs:
            got = hysteria_amd.hooked_relay_acl_decisions(rs, sniffer, ds)
            plain = hysteria_amd.relay_acl_decisions(rs, ds)
            want, rewritten = [], 0
            for d in ds:
                m = udpmsg_ref.parse(d)
                if isinstance(m, int):
                    want.append(None)
                    continue
                chk = R.check(m.addr, True, rewrite_domain, None, udp_ports)
                st, payload = qc.oracle_read(m.data)
                sst, nlen, noff, _, name = sni_ref.quic_sniff(None if st else payload)
                rst, text, rew = R.rewrite(m.addr, chk, name, sst)
                r = A.parse(text) if rst == R.OK else None
                if r is None or r[0] != A.OK:
                    want.append(None)
                    continue
                rewritten += rew
                st, no, nl, v4, v6, fl, port = r
                want.append(rs.decision(rs.match_host(text[no:no + nl], v4 if fl & 1 else None, v6 if fl & 2 else None,
                                                      acl.PROTO_UDP, port)))
            assert got == want
            assert rewritten >= 4 and got != plain          # the hook changes decisions
            assert [g is None for g in got] == [p is None for p in plain]   # and refuses exactly what the plain chain refuses
            assert hysteria_amd.hooked_relay_acl_decisions(rs, sniffer, []) == []
