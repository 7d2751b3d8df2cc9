"""The sniffer's HTTP branch and TCP dispatch on the GPU (hysteria_amd/csrc/
sniff_http.h, sniff.hip, include/hyobfs_sniff.h) against the restatement of
their rules (tests/http_ref.py, pinned in tests/test_http_sniff.py to
sniff_test.go:47-52, :74-77)."""
import base64
import json
import os

import numpy as np
import pytest

import acl_cases as ac
import acl_ref
import http_cases as hc
import http_ref
import sni_ref
import sniff_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64   # sentinel bytes on either side of `names` and of `res`


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Out:
    """`names` (n rows of `stride` bytes) and `res` (n records), each with GUARD
    sentinel bytes before and after."""

    def __init__(self, dev, n, stride):
        self.n, self.stride = n, stride
        self.nbuf = torch.full((2 * GUARD + n * stride,), hc.SENTINEL, dtype=torch.uint8, device=dev)
        self.rbuf = torch.full((2 * GUARD + n * 16,), 0xFF, dtype=torch.uint8, device=dev)
        self.names = self.nbuf[GUARD:GUARD + n * stride] if n * stride else self.nbuf[GUARD:GUARD + 1]
        self.res = self.rbuf[GUARD:GUARD + n * 16]

    def read(self):
        """(records, names as [n, stride]); nothing written outside either."""
        from hysteria_amd import sniff
        nb, rb = self.nbuf.cpu().numpy(), self.rbuf.cpu().numpy()
        end = GUARD + self.n * self.stride
        assert (nb[:GUARD] == hc.SENTINEL).all() and (nb[end:] == hc.SENTINEL).all(), "write outside names"
        assert (rb[:GUARD] == 0xFF).all() and (rb[GUARD + self.n * 16:] == 0xFF).all(), "write outside res"
        return (np.frombuffer(rb[GUARD:GUARD + self.n * 16].tobytes(), sniff.SNIFF_RESULT_DTYPE),
                nb[GUARD:end].reshape(self.n, self.stride))


def _run(dev, call, msgs, stride=hc.NAME_STRIDE):
    buf, off, lens = sc.pack(msgs, gap=3)
    o = Out(dev, len(msgs), stride)
    call(_t(dev, buf), _t(dev, off), _t(dev, lens), len(msgs), o.names, stride, o.res)
    return o.read()


def _check(labels, exp, res, names):
    """status, name_len, name_off, need, the name bytes and the sentinel everywhere
    else in `names`, per stream."""
    stride = names.shape[1]
    assert len(res) == len(exp) == len(names)
    for i, (label, e) in enumerate(zip(labels, exp)):
        r = res[i]
        got = (int(r["status"]), int(r["name_len"]), int(r["name_off"]), int(r["need"]))
        assert got == e[:4], (label, got, e[:4])
        assert names[i].tobytes() == e[4] + bytes([hc.SENTINEL]) * (stride - len(e[4])), label


def _both(dev, cases, stride=hc.NAME_STRIDE):
    from hysteria_amd import sniff
    labels, msgs = [n for n, _ in cases], [m for _, m in cases]
    _check(labels, hc.expected(cases, http_ref.http_request_host, stride),
           *_run(dev, sniff.http_request_host_batch, msgs, stride))
    _check(labels, hc.expected(cases, http_ref.tcp_sniff, stride), *_run(dev, sniff.tcp_sniff_batch, msgs, stride))


def test_lattice_cases(dev):
    """One accepting and one rejecting case per clause of H0-H7, through both entry points."""
    _both(dev, list(hc.lattice_cases()))


def test_window_cases(dev):
    """Line ends, CR LF pairs, the colon, the key and the value at the edges of a
    64-byte step and of a 1024-byte stage; the end of the input; the 256 KiB limit."""
    _both(dev, list(hc.window_cases()))


def test_fuzz_cases(dev):
    """The 512 seeded mutations through both entry points."""
    _both(dev, list(hc.fuzz_cases()))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_name_stride(dev, delta):
    """name_stride one below, at and one above a 5-byte name."""
    by_name = dict(hc.lattice_cases())
    _both(dev, [(n, by_name[n]) for n in hc.STRIDE_CASES], 5 + delta)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_batch_sizes(dev, n):
    """A partial group of four, one group, one stream past it, 64 groups and one."""
    allc = hc.all_cases()
    allc = [c for c in allc if len(c[1]) < 4096]
    _both(dev, [allc[(7 + 13 * k) % len(allc)] for k in range(n)], 64)


def test_batch_above_the_grid_cap(dev):
    """More streams than one pass of the grid takes (65536 workgroups of four):
    prefixes of 10 to 48 bytes, so every wave takes a second stream of another
    kind and the last group of the second pass is partial.  Both entry points."""
    from hysteria_amd import sniff
    temps = hc.small_templates()
    n = hc.GRID_CAP_MSGS + 259
    rng = np.random.default_rng(43)
    pick = rng.integers(0, len(temps), n)
    second = np.arange(hc.GRID_CAP_MSGS, n)
    pick[second] = (pick[second - hc.GRID_CAP_MSGS] + 1 + rng.integers(0, len(temps) - 1, len(second))) % len(temps)
    assert (pick[second] != pick[second - hc.GRID_CAP_MSGS]).all()
    slot, stride = 48, 4
    rows = np.full((len(temps), slot), hc.SENTINEL, np.uint8)
    for k, t in enumerate(temps):
        rows[k, :len(t)] = np.frombuffer(t, np.uint8)
    d_buf = _t(dev, rows[pick].reshape(-1))
    d_off = _t(dev, np.arange(n, dtype=np.uint64) * np.uint64(slot))
    d_len = _t(dev, np.array([len(t) for t in temps], np.uint32)[pick])
    for call, fn in ((sniff.http_request_host_batch, http_ref.http_request_host), (sniff.tcp_sniff_batch, http_ref.tcp_sniff)):
        exp_t = [fn(t, stride) for t in temps]
        assert {e[0] for e in exp_t} >= {0, http_ref.MALFORMED, http_ref.HOST, http_ref.NEED_MORE, http_ref.NAME_CAP}
        o = Out(dev, n, stride)
        call(d_buf, d_off, d_len, n, o.names, stride, o.res)
        res, got = o.read()
        for j, f in enumerate(("status", "name_len", "name_off", "need")):
            want = np.array([e[j] for e in exp_t])[pick]
            bad = np.nonzero(res[f] != want)[0]
            assert not len(bad), (f, int(bad[0]), int(pick[bad[0]]))
        want_rows = np.full((len(temps), stride), hc.SENTINEL, np.uint8)
        for k, e in enumerate(exp_t):
            want_rows[k, :len(e[4])] = np.frombuffer(e[4], np.uint8)
        bad = np.nonzero((got != want_rows[pick]).any(axis=1))[0]
        assert not len(bad), ("names", int(bad[0]), int(pick[bad[0]]))


def test_mixed_batch(dev):
    """HTTP, TLS-record and unrecognised prefixes interleaved, so the waves of one
    workgroup take different branches: every item as the restatement says, and
    every TLS item byte-equal to what hyobfs_tls_record_sni_batch leaves."""
    from hysteria_amd import sniff
    cases = list(hc.mixed_cases())
    labels, msgs = [n for n, _ in cases], [m for _, m in cases]
    res, names = _run(dev, sniff.tcp_sniff_batch, msgs)
    _check(labels, hc.expected(cases, http_ref.tcp_sniff), res, names)
    res2, names2 = _run(dev, sniff.tls_record_sni_batch, msgs)
    tls = [i for i, m in enumerate(msgs) if sni_ref.is_tls(m)]
    assert len(tls) >= 80
    assert res[tls].tobytes() == res2[tls].tobytes() and np.array_equal(names[tls], names2[tls])
    rest = [i for i in range(len(msgs)) if i not in set(tls)]
    assert (res2[rest]["status"] == sni_ref.NOT_TLS).all()


def test_reference_vectors_through_sniffer(dev):
    """TestSnifferTCP's three inputs (sniff_test.go:47-93) through Sniffer.tcp_many,
    next to inputs the sniffer must leave alone."""
    from hysteria_amd import Sniffer, sniff
    with open(os.path.join(ROOT, "tests", "golden", "http_sniff_vectors.json")) as f:
        h1, h2 = json.load(f)["http"]
    with open(os.path.join(ROOT, "tests", "golden", "sniff_vectors.json")) as f:
        t = json.load(f)["tls_record"]
    tls = base64.b64decode(t["data_b64"])
    p1, p2 = h1["data"].encode("latin-1"), h2["data"].encode("latin-1")
    s = Sniffer(timeout=1.0, rewrite_domain=False)
    assert s.tcp_many([p1, p2, tls], [h1["req_addr"], h2["req_addr"], "222.222.222.222:443"]) == \
        ["example.com:80", "example.com:10086", "ipinfo.io:443"]
    assert h1["rewritten"] == "example.com:80" and h2["rewritten"] == "example.com:10086"
    got = s.tcp_many([b"Wait It's All Ohio? Always Has Been.", b"\x01\x02\x03\x04\x05", p1, p1[:30], p2, tls, tls[:100],
                      hc.req(b"GET http://other.example/ HTTP/1.1"), hc.req(headers=(b"User-Agent: x",))],
                     ["123.123.123.123:123", "45.45.45.45:45", "example.org:80", "7.7.7.7:80", "[2001:db8::1]:8080",
                      "@internal", "8.8.8.8:443", "9.9.9.9:80", "6.6.6.6:80"])
    assert got == ["123.123.123.123:123", "45.45.45.45:45", "example.org:80", "7.7.7.7:80", "example.com:8080",
                   "@internal", "8.8.8.8:443", "9.9.9.9:80", "6.6.6.6:80"]
    assert s.tcp_many([], []) == []
    got = sniff.http_request_hosts([p2, tls, p1[:30], hc.req(b"CONNECT a:1 HTTP/1.1")])
    assert got[0] == b"example.com"
    assert [g.status for g in got[1:]] == [sniff.ERR_NOT_HTTP, sniff.ERR_NEED_MORE, sniff.ERR_HOST]
    got = sniff.tcp_snis([p1, tls, b"\x00\x00\x00", b"ab"])
    assert got[:2] == [b"example.com", b"ipinfo.io"]
    assert [g.status for g in got[2:]] == [sniff.ERR_UNRECOGNIZED, sniff.ERR_NEED_MORE]


SNIFF_RULES = [ac.R("suffix", 21, pattern=b"example.com", hijack=3), ac.R("wildcard", 22, pattern=b"*.example.net"),
               ac.R("exact", 23, pattern=b"a", proto=1, ports=(80, 80)), ac.R("all", 24, proto=1)]


def test_sniff_then_acl(dev):
    """hyobfs_acl_match_sniffed_batch over what hyobfs_tcp_sniff_batch left in
    `names` and `res` for the lattice, the small window cases and some fuzz
    cases: the decisions are acl_ref's over the restatement's names."""
    from hysteria_amd import acl, sniff
    cases = list(hc.lattice_cases()) + list(hc.small_window_cases()) + list(hc.fuzz_cases())[:128]
    msgs = [m for _, m in cases]
    n, stride = len(cases), hc.NAME_STRIDE
    sniffed = hc.expected(cases, http_ref.tcp_sniff, stride)
    items = [ac.item(e[4], None, None, 1, 80 if i % 3 else 8080) for i, e in enumerate(sniffed)]
    buf, off, lens = sc.pack(msgs, gap=3)
    o = Out(dev, n, stride)
    sniff.tcp_sniff_batch(_t(dev, buf), _t(dev, off), _t(dev, lens), n, o.names, stride, o.res)
    _, _, _, _, _, _, proto, port = (_t(dev, a) for a in ac.arrays(items))
    arr, keep = ac.c_rules(SNIFF_RULES)
    h = acl.ruleset_new(arr, len(SNIFF_RULES), 0)
    try:
        d_acl = torch.full((2 * GUARD + 16 * n,), 0xA5, dtype=torch.uint8, device=dev)
        acl.match_sniffed_batch(h, o.names, stride, o.res, None, None, None, proto, port, n, d_acl[GUARD:GUARD + 16 * n])
        raw = d_acl.cpu().numpy()
    finally:
        acl.ruleset_free(h)
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + 16 * n:] == 0xA5).all()
    got = np.frombuffer(raw[GUARD:GUARD + 16 * n].tobytes(), acl.ACL_RESULT_DTYPE)
    exp = [acl_ref.expected(SNIFF_RULES, it, e[0]) for it, e in zip(items, sniffed)]
    for i, (g, e) in enumerate(zip(got, exp)):
        g = (int(g["status"]), int(g["rule"]), int(g["outbound"]), int(g["hijack"]))
        assert g == e, (cases[i][0], g, e)
    kinds = [e[0] for e in exp]
    assert kinds.count(acl_ref.NO_NAME) >= 60 and kinds.count(0) >= 100, kinds
    assert {e[2] for e in exp} >= {21, 22, 23, 24}
