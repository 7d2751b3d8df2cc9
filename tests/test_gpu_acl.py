"""The ACL matcher on the GPU (hysteria_amd/csrc/acl.hip, include/hyobfs_acl.h)
against the restatement of the reference's Match and matchers (tests/acl_ref.py,
pinned in tests/test_acl.py to matchers_test.go, compile_test.go and
parse_test.go)."""
import base64
import ipaddress
import json
import os

import numpy as np
import pytest

import acl_cases as ac
import acl_ref
import quic_cases as qc
import sni_ref
import sniff_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64   # sentinel bytes on either side of `res`


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _vectors(name):
    with open(os.path.join(ROOT, "tests", "golden", name), encoding="utf-8") as f:
        return json.load(f)


def _t(dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


class Res:
    """n result records with GUARD sentinel bytes before and after them."""

    def __init__(self, dev, n):
        self.n = n
        self.buf = torch.full((2 * GUARD + 16 * n,), 0xA5, dtype=torch.uint8, device=dev)
        self.res = self.buf[GUARD:GUARD + 16 * n]

    def records(self):
        from hysteria_amd import acl
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + 16 * self.n:] == 0xA5).all(), "write outside res"
        return np.frombuffer(h[GUARD:GUARD + 16 * self.n].tobytes(), acl.ACL_RESULT_DTYPE)


class Set:
    """A device rule set made from the cases' rule dicts."""

    def __init__(self, rules, device=0):
        from hysteria_amd import acl
        arr, self.keep = ac.c_rules(rules)
        self.h = acl.ruleset_new(arr, len(rules), device)

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        from hysteria_amd import acl
        acl.ruleset_free(self.h)


def _same(label, items, got, exp):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        g = (int(g["status"]), int(g["rule"]), int(g["outbound"]), int(g["hijack"]))
        assert g == e, (label, i, items[i] if items is not None else None, g, e)


def test_case_families(dev):
    """Every case family of tests/acl_cases.py, the whole balanced random set
    included, through hyobfs_acl_match_batch; nothing written outside res."""
    from hysteria_amd import acl
    groups = ac.all_groups()
    assert sum(len(g[2]) for g in groups) > 3000
    for label, rules, items in groups:
        with Set(rules) as h:
            names, off, lens, v4, v6, fl, proto, port = (_t(dev, a) for a in ac.arrays(items))
            r = Res(dev, len(items))
            acl.match_batch(h, names, off, lens, v4, v6, fl, proto, port, len(items), r.res)
            _same(label, items, r.records(), ac.expected((label, rules, items)))


def test_null_addresses_and_empty_batch(dev):
    """ip_flags / ipv4 / ipv6 null: no item has an address; n == 0 launches nothing."""
    from hysteria_amd import acl
    label, rules, items = ac.cidr_set_groups()[1]   # size_0, inverse: every item without an address matches
    items = [(it[0], None, None, it[3], it[4]) for it in items]
    with Set(rules) as h:
        names, off, lens, _, _, _, proto, port = (_t(dev, a) for a in ac.arrays(items))
        r = Res(dev, len(items))
        acl.match_batch(h, names, off, lens, None, None, None, proto, port, len(items), r.res)
        _same(label, items, r.records(), ac.expected((label, rules, items)))
        r = Res(dev, 1)
        acl.match_batch(h, names, off, lens, None, None, None, proto, port, 0, r.res)
        assert (r.buf.cpu().numpy() == 0xA5).all()


SNIFF_RULES = [ac.R("exact", 11, pattern=b"www.notion.so", hijack=2), ac.R("suffix", 12, pattern=b"ipinfo.io"),
               ac.R("suffix", 13, pattern=b"example.org", proto=2, ports=(443, 443)),
               ac.R("cidr", 14, ip=ac.ip("10.9.0.0"), prefix=16), ac.R("wildcard", 15, pattern=b"*.*", proto=2),
               ac.R("all", 16, proto=1)]


def test_match_sniffed_over_the_sniffer_output(dev):
    """hyobfs_acl_match_sniffed_batch over what hyobfs_quic_sniff_batch left in
    `names` and `sres` for the sniffer's own case packets and the reference's
    www.notion.so Initial (sniff_test.go:133-139), on one stream; then over
    hyobfs_tls_record_sni_batch's output for the reference's ipinfo.io record
    (sniff_test.go:86-93).  What must come out is the restatements' alone:
    sni_ref for the names, acl_ref for the decisions."""
    from hysteria_amd import acl, sniff
    vec = _vectors("sniff_vectors.json")
    cases = list(sc.quic_cases(False))
    pkts = [p for _, p, _ in cases] + [base64.b64decode(vec["quic_initial"]["data_b64"])]
    sniffed = sc.expected_quic(cases) + [(0, 13, 0, 0, b"www.notion.so")]
    n, cap, stride = len(pkts), 2048, sc.NAME_STRIDE
    items = [ac.item(e[4], "10.9.%d.1" % (i % 7) if i % 5 == 0 else None, None, 2, 443 if i % 3 else 8443)
             for i, e in enumerate(sniffed)]
    buf, off, lens = qc.pack(pkts)
    d_names = torch.full((n * stride + 64,), sc.SENTINEL, dtype=torch.uint8, device=dev)
    d_sres = torch.full((n * 16,), 0xFF, dtype=torch.uint8, device=dev)
    d_crypto = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    d_qres = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    ws = torch.empty(sniff.quic_sniff_workspace_size(n), dtype=torch.uint8, device=dev)
    _, _, _, v4, v6, fl, proto, port = (_t(dev, a) for a in ac.arrays(items))
    with Set(SNIFF_RULES) as h:
        r = Res(dev, n)
        sniff.quic_sniff_batch(_t(dev, buf), _t(dev, off), _t(dev, lens), n, d_crypto,
                               _t(dev, np.arange(n, dtype=np.uint64) * np.uint64(cap)),
                               _t(dev, np.full(n, cap, np.uint32)), d_qres, d_names, stride, d_sres, ws)
        acl.match_sniffed_batch(h, d_names, stride, d_sres, v4, v6, fl, proto, port, n, r.res)
        got = r.records()
        sres = np.frombuffer(d_sres.cpu().numpy().tobytes(), sniff.SNIFF_RESULT_DTYPE)
        assert [int(s) for s in sres["status"]] == [e[0] for e in sniffed]
        exp = [acl_ref.expected(SNIFF_RULES, it, e[0]) for it, e in zip(items, sniffed)]
        _same("quic_sniff", items, got, exp)
        assert exp[-1] == (0, 0, 11, 2)
        kinds = [e[0] for e in exp]
        assert kinds.count(acl_ref.NO_NAME) >= 20 and kinds.count(0) >= 40, kinds   # packets without a name
        assert {e[2] for e in exp} >= {0, 11, 13, 14, 15}
        # the TLS branch: the reference's record, a cut one (NEED_MORE), no TLS at all, a record without a name
        tls = base64.b64decode(vec["tls_record"]["data_b64"])
        by_name = dict(sc.generator_cases())
        msgs = [tls, tls[:100], b"GET / HTTP/1.1\r\n", sc.as_record(by_name["no_type_0"]), sc.as_record(by_name["valid"])]
        sniffed = [sni_ref.tls_record_sni(m, stride) for m in msgs]
        items = [ac.item(e[4], None, None, 1, 443) for e in sniffed]
        buf, off, lens = sc.pack(msgs, gap=3)
        m = len(msgs)
        d_names.fill_(sc.SENTINEL)
        sniff.tls_record_sni_batch(_t(dev, buf), _t(dev, off), _t(dev, lens), m, d_names, stride, d_sres)
        _, _, _, _, _, _, proto, port = (_t(dev, a) for a in ac.arrays(items))
        r = Res(dev, m)
        acl.match_sniffed_batch(h, d_names, stride, d_sres, None, None, None, proto, port, m, r.res)
        exp = [acl_ref.expected(SNIFF_RULES, it, e[0]) for it, e in zip(items, sniffed)]
        _same("tls_record", items, r.records(), exp)
        assert [e[:3] for e in exp] == [(0, 1, 12), (acl_ref.NO_NAME, -1, 0), (acl_ref.NO_NAME, -1, 0),
                                        (acl_ref.NO_NAME, -1, 0), (0, 5, 16)]


def test_one_rule_set_two_streams(dev):
    """One rule set, two batches on two streams at once."""
    from hysteria_amd import acl
    label, rules, items = ac.random_group()
    halves = (items[:1024], items[1024:])
    with Set(rules) as h:
        streams = [torch.cuda.Stream(dev) for _ in halves]
        args = [[_t(dev, a) for a in ac.arrays(half)] for half in halves]
        res = [Res(dev, len(half)) for half in halves]
        torch.cuda.synchronize(dev)
        for s, a, r, half in zip(streams, args, res, halves):
            acl.match_batch(h, *a, len(half), r.res, stream=s)
        for s in streams:
            s.synchronize()
        for r, half in zip(res, halves):
            _same(label, half, r.records(), ac.expected((label, rules, half)))


def test_batch_above_the_grid_cap(dev):
    """One item more than a full pass of the capped grid (65536 workgroups of
    four), cycling 61 items of the random set (61 and 4 share no factor, so every
    wave position sees every item): the first wave's stride loop runs once."""
    from hysteria_amd import acl
    label, rules, items = ac.random_group()
    items = items[:61]
    exp = np.array(ac.expected((label, rules, items)), np.int64)
    assert len({tuple(e) for e in exp}) > 20
    n = ac.GRID_CAP_ITEMS + 1
    pick = np.arange(n) % len(items)
    slot = 64
    assert max(len(it[0]) for it in items) <= slot
    rows = np.full((len(items), slot), 0xA5, np.uint8)
    for k, it in enumerate(items):
        rows[k, :len(it[0])] = np.frombuffer(it[0], np.uint8)
    _, _, lens, v4, v6, fl, proto, port = ac.arrays(items)
    with Set(rules) as h:
        r = Res(dev, n)
        acl.match_batch(h, _t(dev, rows.reshape(-1)), _t(dev, pick.astype(np.uint64) * np.uint64(slot)),
                        _t(dev, lens[pick]), _t(dev, v4.reshape(-1, 4)[pick].reshape(-1)),
                        _t(dev, v6.reshape(-1, 16)[pick].reshape(-1)), _t(dev, fl[pick]), _t(dev, proto[pick]),
                        _t(dev, port[pick]), n, r.res)
        got = r.records()
    for j, f in enumerate(("status", "rule", "outbound", "hijack")):
        bad = np.nonzero(got[f].astype(np.int64) != exp[pick, j])[0]
        assert not len(bad), (f, int(bad[0]), int(pick[bad[0]]))


class Geo:
    def __init__(self, v):
        self.v = v

    def geoip(self, code):
        g = self.v["geoip"].get(code)
        return None if g is None else ([(ipaddress.ip_address(a).packed, p) for a, p in g["cidrs"]], g["inverse"])

    def geosite(self, name):
        g = self.v["geosite"].get(name)
        return None if g is None else [tuple(e) for e in g]


def test_match_many_on_the_compile_table(dev):
    """TestCompile (compile_test.go:25-346) end to end: text rules compiled, the
    table's hosts (trailing-dot rows included) through RuleSet.match_many; then
    IDN rules, whose names the device leaves to the host matcher."""
    import hysteria_amd
    v = _vectors("acl_vectors.json")["compile"]
    text = "\n".join("%s(%s)" % (r["outbound"], ", ".join(x for x in (r["address"], r["proto_port"] or "*",
                                                                      r["hijack_address"]) if x)) for r in v["rules"])
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(text), v["outbounds"], Geo(v)) as rs:
        tests = v["tests"]
        got = rs.match_many([(t["name"], t["ipv4"], t["ipv6"]) for t in tests], [t["proto"] for t in tests],
                            [t["port"] for t in tests])
        assert got == [(t["want_outbound"], t["want_ip"]) for t in tests]
        assert rs.match_many([], [], []) == []
    idn = "a(政府.中国)\nb(*大学*, tcp)\nc(suffix:中国)\nd(all, udp)"
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(idn), {"a": 1, "b": 2, "c": 3, "d": 4}) as rs:
        hosts = ["xn--mxtq1m.xn--fiqs8s", "xn--mxtq1m.xn--yfro4i67o", "xn--xkry9kk1bz66a.xn--ses554g", "天安门.中国.",
                 "plain.example", "XN--MXTQ1M.xn--FIQS8S."]
        got = rs.match_many([(h, None, None) for h in hosts], [1] * 6, [443] * 6)
        assert [g[0] for g in got] == [1, 0, 2, 3, 0, 1]
        assert [g[0] for g in rs.match_many([(h, None, None) for h in hosts], [2] * 6, [443] * 6)] == [1, 4, 4, 3, 4, 1]


def test_quic_sniff_and_match(dev):
    """The fused example: datagrams in, decisions out; None where the sniffer finds
    no name."""
    import hysteria_amd
    vec = _vectors("sniff_vectors.json")
    by_name = dict(sc.generator_cases())
    pkt = base64.b64decode(vec["quic_initial"]["data_b64"])
    text = "direct(suffix:notion.so, udp/443, 9.9.9.9)\nproxy(example.org)\nblock(10.0.0.0/8)\nlast(all, udp/8443)"
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(text),
                                    {"direct": 1, "proxy": 2, "block": 3, "last": 4}) as rs:
        got = hysteria_amd.quic_sniff_and_match(
            rs, [pkt, sc.initial_for(by_name["valid"], 1), b"\x01\x02\x03", pkt, sc.initial_for(by_name["no_type_0"], 2),
                 sc.initial_for(by_name["valid"], 3)],
            [443, 443, 443, 8443, 443, 8443], hosts=[(None, None), ("10.1.2.3", None)] + [(None, None)] * 4)
        assert got == [(1, "9.9.9.9"), (2, None), None, (4, None), None, (2, None)]
        assert hysteria_amd.quic_sniff_and_match(rs, [], []) == []
