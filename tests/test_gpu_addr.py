"""The request-address kernels on the GPU (hysteria_amd/csrc/addr.hip,
include/hyobfs_addr.h): the lattice of tests/addr_cases.py through the three device
calls, bit-exact against the restatement (tests/addr_ref.py), every output array
between guard bytes and every input in poisoned surroundings; the addresses of relay
datagrams; the chain relay datagram -> ACL decision; and the reply chain format ->
fragment -> parse -> address on the device."""
import numpy as np
import pytest

import addr_cases as ac
import addr_ref as R
import udpmsg_ref
from test_addr import check_parse_udp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = ac.GUARD_BYTES   # guard bytes (0xA5) on both sides of every output array


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)   # a writable copy


class Guarded:
    """nbytes of device memory between two runs of PAD guard bytes; the payload starts
    `mis` bytes past a 16-byte boundary."""

    def __init__(self, dev, nbytes, mis=0):
        self.lead, self.nbytes = PAD + mis, nbytes   # torch allocations are at least 256-aligned
        self.t = torch.full((self.lead + nbytes + PAD,), ac.GUARD, dtype=torch.uint8, device=dev)
        assert self.t.data_ptr() % 16 == 0 and PAD % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead

    def read(self, dtype=np.uint8):
        """The payload, after checking that both guards are intact."""
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == ac.GUARD).all() and (h[self.lead + self.nbytes:] == ac.GUARD).all(), "guard bytes"
        return np.frombuffer(h[self.lead:self.lead + self.nbytes].tobytes(), dtype)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def parse_outputs(dev, n):
    mis = n % 4
    return {name: Guarded(dev, n * w * np.dtype(dt).itemsize, mis if name in ("ipv4", "ipv6") else 0)
            for name, dt, w in ac.PARSE_OUT}


def read_outputs(out):
    return {name: out[name].read(dt) for name, dt, _ in ac.PARSE_OUT}


def run_parse(dev, buf: bytes, off, lens):
    from hysteria_amd import addr
    n = len(off)
    d_buf = _t(dev, np.frombuffer(buf + b":", np.uint8))
    d_off, d_len = _t(dev, np.array(off, np.uint64)), _t(dev, np.array(lens, np.uint32))
    out = parse_outputs(dev, n)
    rc = addr._adlib().hyobfs_addr_parse_batch(d_buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                               *(out[name].ptr for name, _, _ in ac.PARSE_OUT), _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0
    return read_outputs(out)


@pytest.mark.parametrize("case", ac.parse_cases(), ids=[c["name"] for c in ac.parse_cases()])
def test_parse_lattice(dev, case):
    buf, off, lens = ac.layout(case)
    ac.check_parse(case["name"], case["items"], off, run_parse(dev, buf, off, lens))


def test_parse_udp(dev):
    from hysteria_amd import addr, udpmsg
    ds, addrs, at = ac.udp_datagrams()
    buf, off, lens = ac.layout(dict(items=ds, mode="poison"))
    n = len(ds)
    d_buf = _t(dev, np.frombuffer(buf, np.uint8))
    d_off, d_len = _t(dev, np.array(off, np.uint64)), _t(dev, np.array(lens, np.uint32))
    d_parsed = torch.zeros(n * udpmsg.PARSED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    udpmsg.parse_batch(d_buf, d_off, d_len, n, d_parsed)
    out = parse_outputs(dev, n)
    rc = addr._adlib().hyobfs_addr_parse_udp_batch(d_buf.data_ptr(), d_off.data_ptr(), d_parsed.data_ptr(), n,
                                                   *(out[name].ptr for name, _, _ in ac.PARSE_OUT), _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0
    recs = np.frombuffer(d_parsed.cpu().numpy().tobytes(), udpmsg.PARSED_DTYPE)
    assert [int(r["status"]) == 0 for r in recs] == [a is not None for a in addrs]
    check_parse_udp(addrs, [o + a for o, a in zip(off, at)], read_outputs(out))


def run_format(dev, case, base_off=ac.BASE_OFF):
    from hysteria_amd import addr
    n, stride, mis = len(case["items"]), case["stride"], case["mis"]
    ip = np.frombuffer(bytes(mis) + b"".join(x[0] for x in case["items"]), np.uint8)
    d_ip = _t(dev, ip)
    d_fam = _t(dev, np.array([x[1] for x in case["items"]], np.uint8))
    d_port = _t(dev, np.array([x[2] for x in case["items"]], np.uint16).view(np.int16))
    status, out_len, out = Guarded(dev, 4 * n), Guarded(dev, 4 * n), Guarded(dev, n * stride, mis)
    meta = Guarded(dev, n * ac.META_DTYPE.itemsize) if case["meta"] else None
    rc = addr._adlib().hyobfs_addr_format_batch(d_ip.data_ptr() + mis, d_fam.data_ptr(), d_port.data_ptr(), n, out.ptr, stride,
                                                base_off, out_len.ptr, meta.ptr if meta else None, status.ptr, _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0
    return status.read(np.int32), out_len.read(np.uint32), meta.read(ac.META_DTYPE) if meta else None, out.read()


@pytest.mark.parametrize("case", ac.format_cases(), ids=[c["name"] for c in ac.format_cases()])
def test_format_lattice(dev, case):
    ac.check_format(case, *run_format(dev, case))


RULES = """
pinned(1.2.3.4)
lan(10.0.0.0/8)
site(suffix:example.com, *, 9.9.9.9)
reject(suffix:bad.test)
idn(政府.中国)
games(all, udp/1000-2000)
"""
OUTBOUNDS = {"pinned": 1, "lan": 2, "site": 3, "reject": 4, "idn": 5, "games": 6}
CHAIN_ADDRS = [b"1.2.3.4:53", b"[::ffff:1.2.3.4]:9", b"[::ffff:10.1.2.3]:80", b"10.9.9.9:1", b"[::10.1.2.3]:80",
               b"www.example.com:443", b"example.com:0443", b"EXAMPLE.COM.:443", b"x.bad.test:80", b"other.org:1500",
               b"other.org:2001", b"[2001:db8::1]:1999", b"[2001:db8::1]:999", b"nocolon", b"h:65536", b"a:b:1",
               b"[::1]x:1", b"xn--mxtq1m.xn--fiqs8s:443", b"11.0.0.1:1000", b"1.2.3.4.5:1000", b"[fe80::1%eth0]:1000"]


def test_relay_acl_decisions(dev):
    import hysteria_amd
    from hysteria_amd import acl
    ds = [ac.datagram(a, data=b"payload") for a in CHAIN_ADDRS]
    ds.insert(3, bytes(5))                      # a message that does not parse
    ds.insert(9, ac.datagram(b"a:1", data=b""))  # no data byte: refused by the message parser
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(RULES), OUTBOUNDS) as rs:
        got = hysteria_amd.relay_acl_decisions(rs, ds)
        want = []
        for d in ds:
            m = udpmsg_ref.parse(d)
            r = None if isinstance(m, int) else R.parse(m.addr)
            if r is None or r[0] != R.OK:
                want.append(None)
                continue
            st, no, nl, v4, v6, fl, port = r
            want.append(rs.decision(rs.match_host(m.addr[no:no + nl], v4 if fl & 1 else None, v6 if fl & 2 else None,
                                                  acl.PROTO_UDP, port)))
        assert got == want
        assert hysteria_amd.relay_acl_decisions(rs, []) == []
    by_addr = dict(zip(CHAIN_ADDRS, [g for i, g in enumerate(got) if i not in (3, 9)]))
    assert by_addr[b"1.2.3.4:53"] == by_addr[b"[::ffff:1.2.3.4]:9"] == (1, None)
    assert by_addr[b"[::ffff:10.1.2.3]:80"] == by_addr[b"10.9.9.9:1"] == (2, None)   # the v4 CIDR holds the mapped literal
    assert by_addr[b"[::10.1.2.3]:80"] == (0, None)                                    # the compatible form is IPv6
    assert by_addr[b"www.example.com:443"] == by_addr[b"example.com:0443"] == (3, "9.9.9.9")
    assert by_addr[b"x.bad.test:80"] == (4, None) and by_addr[b"xn--mxtq1m.xn--fiqs8s:443"] == (5, None)
    assert by_addr[b"other.org:1500"] == by_addr[b"[2001:db8::1]:1999"] == by_addr[b"11.0.0.1:1000"] == (6, None)
    assert by_addr[b"other.org:2001"] == by_addr[b"[2001:db8::1]:999"] == (0, None)
    assert by_addr[b"1.2.3.4.5:1000"] == by_addr[b"[fe80::1%eth0]:1000"] == (6, None)   # names, not addresses
    assert [by_addr[a] for a in (b"nocolon", b"h:65536", b"a:b:1", b"[::1]x:1")] == [None] * 4
    assert got[3] is None and got[9] is None


def test_reply_chain_on_the_device(dev):
    """format_batch with meta -> hyobfs_udp_frag_batch -> hyobfs_udp_parse_batch -> parse_udp_batch: every
    (address, port) comes back, without the texts ever leaving the device."""
    from hysteria_amd import addr, udpmsg
    items = [x for x in ac.format_items() if x[1] in (4, 16)]
    n, stride = len(items), 48
    meta = np.zeros(n, udpmsg.META_DTYPE)
    meta["session_id"], meta["packet_id"], meta["max_size"] = np.arange(n) + 7, 1, 1200
    meta["addr_off"], meta["addr_len"] = 0xDEAD, 0xBEEF   # format_batch fills these
    d_meta = _t(dev, meta.view(np.uint8))
    d_ip = _t(dev, np.frombuffer(b"".join(x[0] for x in items), np.uint8))
    d_fam = _t(dev, np.array([x[1] for x in items], np.uint8))
    d_port = _t(dev, np.array([x[2] for x in items], np.uint16).view(np.int16))
    d_texts = torch.full((n * stride,), 0xEE, dtype=torch.uint8, device=dev)
    d_tlen = torch.zeros(n, dtype=torch.int32, device=dev)
    d_fst = torch.zeros(n, dtype=torch.int32, device=dev)
    addr.format_batch(d_ip, d_fam, d_port, n, d_texts, stride, 0, d_tlen, d_meta, d_fst)
    payload = 24
    d_data = torch.full((n * payload,), ord("]"), dtype=torch.uint8, device=dev)
    d_doff = _t(dev, np.arange(n, dtype=np.uint64) * np.uint64(payload))
    d_dlen = _t(dev, np.full(n, payload, np.uint32))
    out_cap = n * (8 + 1 + addr.FORMAT_MAX + payload)
    d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)
    d_goff = torch.zeros(n, dtype=torch.int64, device=dev)
    d_glen = torch.zeros(n, dtype=torch.int32, device=dev)
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sst = torch.zeros(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.zeros(udpmsg.frag_workspace_size(n), dtype=torch.uint8, device=dev)
    udpmsg.frag_batch(d_data, d_doff, d_dlen, d_meta, d_texts, n, d_out, out_cap, d_goff, d_glen, n, d_first, d_sst, d_tot, ws)
    d_parsed = torch.zeros(n * udpmsg.PARSED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    udpmsg.parse_batch(d_out, d_goff, d_glen, n, d_parsed)
    st, noff, nlen, v4, v6, fl, port = addr.parse_outputs(n, dev)
    addr.parse_udp_batch(d_out, d_goff, d_parsed, n, st, noff, nlen, v4, v6, fl, port)
    torch.cuda.synchronize(dev)
    assert not d_fst.any() and not d_sst.any() and int(d_tot[1]) == n and not st.any()
    out, noff, nlen = d_out.cpu().numpy(), noff.cpu().numpy(), nlen.cpu().numpy()
    v4, v6, fl, port = v4.cpu().numpy(), v6.cpu().numpy(), fl.cpu().numpy(), port.cpu().numpy().view(np.uint16)
    for i, (ip, fam, p) in enumerate(items):
        ip16 = R.V4_IN_V6 + ip[:4] if fam == 4 else ip
        host = R.ip_string(ip16)
        assert out[int(noff[i]):int(noff[i]) + int(nlen[i])].tobytes() == host and int(port[i]) == p
        if R.to4(ip16) is not None:
            assert (int(fl[i]), v4[4 * i:4 * i + 4].tobytes(), v6[16 * i:16 * i + 16].tobytes()) == (1, ip16[12:], bytes(16))
        else:
            assert (int(fl[i]), v4[4 * i:4 * i + 4].tobytes(), v6[16 * i:16 * i + 16].tobytes()) == (2, bytes(4), ip16)


def test_refusals_run_no_kernel(dev):
    from hysteria_amd import _lib, addr
    lib, N = addr._adlib(), None
    g = Guarded(dev, 256)
    p = g.ptr
    assert lib.hyobfs_addr_parse_batch(N, N, N, 0, N, N, N, N, N, N, N, N) == 0
    assert lib.hyobfs_addr_parse_udp_batch(N, N, N, 0, N, N, N, N, N, N, N, N) == 0
    assert lib.hyobfs_addr_format_batch(N, N, N, 0, N, 0, 0, N, N, N, N) == 0
    full = [p] * 3 + [1] + [p] * 7 + [_stream(dev)]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10):   # every pointer is required
        args = list(full)
        args[k] = N
        assert lib.hyobfs_addr_parse_batch(*args) == _lib.HYOBFS_ERR_INVALID
        assert lib.hyobfs_addr_parse_udp_batch(*args) == _lib.HYOBFS_ERR_INVALID
    fmt = [p, p, p, 1, p, 47, 0, p, p, p, _stream(dev)]
    for k in (0, 1, 2, 4, 7, 9):   # meta (8) is optional
        args = list(fmt)
        args[k] = N
        assert lib.hyobfs_addr_format_batch(*args) == _lib.HYOBFS_ERR_INVALID
    fmt[5] = 46
    assert lib.hyobfs_addr_format_batch(*fmt) == _lib.HYOBFS_ERR_INVALID
    torch.cuda.synchronize(dev)
    assert (g.read() == ac.GUARD).all()   # nothing ran
