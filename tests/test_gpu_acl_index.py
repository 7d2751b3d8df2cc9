"""The ACL's hashed index over a DOMAIN_SET's FULL and ROOT values on the GPU
(hysteria_amd/csrc/acl.hip, entry kind kDomainIndex: a lane hashes the name in LDS
from its end and looks every label-aligned suffix up in the set's slot table)
through RuleSet.match_batch, match_sniffed_batch and match_many, against the
restatement (tests/acl_ref.py with the regex branch of tests/acl_regex_cases.py).
Every group is also compiled without the index; the two record arrays must be
equal.  The groups are the smallest shapes at which the kernel can go wrong;
tests/test_acl_index.py runs the same ones under AddressSanitizer."""
import numpy as np
import pytest

import acl_cases as ac
import acl_index_cases as ic
import acl_ref
import acl_regex_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64   # sentinel bytes on either side of `res`


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def groups():
    """(group, its rule set with the index, the same rules without) for every group, made once."""
    from hysteria_amd import acl
    out = [(g, acl.RuleSet(ac.product_rules(g[1]), device_index=True, index_min=ic.index_min(g[0])),
            acl.RuleSet(ac.product_rules(g[1]))) for g in ic.groups()]
    yield out
    for _, a, b in out:
        a.close()
        b.close()


def _t(dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _res(dev, n):
    buf = torch.full((2 * GUARD + 16 * n,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + 16 * n]


def _records(buf, n):
    from hysteria_amd import acl
    h = buf.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + 16 * n:] == 0xA5).all(), "write outside res"
    return np.frombuffer(h[GUARD:GUARD + 16 * n].tobytes(), acl.ACL_RESULT_DTYPE)


def _same(label, items, got, exp):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        g = (int(g["status"]), int(g["rule"]), int(g["outbound"]), int(g["hijack"]))
        assert g == e, (label, i, items[i], g, e)


def test_tables(dev, groups):
    """The walk table's entries and each rule's slot table as the cases pin them;
    without the index one entry per value and no table."""
    from hysteria_amd import acl
    for group, rs, lin in groups:
        label, rules, _ = group
        assert rs.flags() & acl.FLAG_INDEX and not lin.flags() & acl.FLAG_INDEX, label
        h, hl = rs.device_set(0), lin.device_set(0)
        assert acl.ruleset_entries(hl) == sum(len(r["entries"]) if r["kind"] == "domain_set" else 1 for r in rules), label
        info = {r: acl.ruleset_index_info(h, r) for r in range(len(rules))}
        assert all(acl.ruleset_index_info(hl, r) == (0, 0, 0) for r in range(len(rules))), label
        for r, (values, slots, probe) in info.items():
            assert slots == 0 or (slots >= 2 * values and slots & (slots - 1) == 0 and 1 <= probe <= values), (label, r)
        if label in ic.SHAPE:
            entries, index = ic.SHAPE[label]
            assert acl.ruleset_entries(h) == entries, label
            assert {r: tuple(v[:2]) for r, v in info.items() if v.slots} == index, label
        if label == "ix_big":
            assert info[0].max_probe >= 2   # chains were walked
        if label == "ix_threshold_65":
            assert info[0].slots == 0 and info[1].slots == 256   # 64 values under the default: not indexed; 65: indexed


def test_match_batch(dev, groups):
    """Every group through RuleSet.match_batch, with the index and without; nothing
    written outside res."""
    for group, rs, lin in groups:
        label, rules, items = group
        names, off, lens, v4, v6, fl, proto, port = (_t(dev, a) for a in ac.arrays(items))
        got = []
        for s in (rs, lin):
            buf, res = _res(dev, len(items))
            s.match_batch(names, off, lens, v4, v6, fl, proto, port, len(items), res, device=0)
            got.append(_records(buf, len(items)))
        _same(label, items, got[0], rc.expected(group))
        assert got[0].tobytes() == got[1].tobytes(), label


def test_match_sniffed_batch(dev, groups):
    """Every group through RuleSet.match_sniffed_batch: names in rows of a stride
    with sentinel bytes after them, every 7th item a failed sniff and every empty
    name NO_NAME."""
    from hysteria_amd import sniff
    stride = ac.SNIFFED_STRIDE
    seen = set()
    for k, (group, rs, lin) in enumerate(groups):
        label, rules, items = group
        n = len(items)
        st = ac.sniff_statuses(items, k)
        rows = np.full((n, stride), 0xA5, np.uint8)
        sres = np.zeros(n, sniff.SNIFF_RESULT_DTYPE)
        for i, it in enumerate(items):
            if st[i] == 0:
                rows[i, :len(it[0])] = np.frombuffer(it[0], np.uint8)
            sres[i] = (st[i], len(it[0]), 7, 0)
        _, _, _, v4, v6, fl, proto, port = (_t(dev, a) for a in ac.arrays(items))
        d_rows, d_sres = _t(dev, rows.reshape(-1)), _t(dev, sres.view(np.uint8))
        got = []
        for s in (rs, lin):
            buf, res = _res(dev, n)
            s.match_sniffed_batch(d_rows, stride, d_sres, v4, v6, fl, proto, port, n, res, device=0)
            got.append(_records(buf, n))
        exp = rc.expected(group, True, k)
        _same(label, items, got[0], exp)
        assert got[0].tobytes() == got[1].tobytes(), label
        seen |= {e[0] for e in exp}
    assert seen == {0, acl_ref.NO_NAME, acl_ref.HOST}


def test_match_many(dev, groups):
    """Every group through RuleSet.match_many: the names the device leaves to the
    host are finished by the host matcher, which knows nothing of the index."""
    for group, rs, lin in groups:
        label, rules, items = group
        got = rs.match_many([it[:3] for it in items], [it[3] for it in items], [it[4] for it in items])
        assert got == lin.match_many([it[:3] for it in items], [it[3] for it in items], [it[4] for it in items]), label
        for it, g in zip(items, got):
            r = rc.match(rules, it[:3], it[3], it[4])
            assert g == ((rules[r]["outbound"], None) if r >= 0 else (0, None)), (label, it, g, r)


def test_refused_value_names_rule_and_entry(dev):
    """A value of 256 bytes in an indexed set: HYOBFS_ACL_ERR_PATTERN with rule and entry."""
    from hysteria_amd import acl
    arr, keep = ac.c_rules([ac.R("all", 1), ac.R("domain_set", 2, entries=[("root", b"a.test"), ("full", b"x" * 256)])])
    with pytest.raises(acl.RuleRefused) as e:
        acl.ruleset_new(arr, 2, 0, acl.FLAG_INDEX, index_min=1)
    assert (e.value.status, e.value.rule, e.value.entry) == (acl.ERR_PATTERN, 1, 1)


def test_compiled_cn_end_to_end(dev):
    """Text rules over the fixture's cn list (200 roots, 37 regexes) through
    compile_rules(..., device_regex=True, device_index=True) and match_many."""
    import hysteria_amd
    from hysteria_amd import acl
    fx = rc.fixture()

    class Geo:
        def geoip(self, code):
            return None

        def geosite(self, name):
            return [("regex", v, a) for n, v, a in fx["entries"] if n == name] + \
                [tuple(e) for e in fx["extra"].get(name, [])] or None

    roots = [e[1] for e in fx["extra"]["cn"]]
    sample = fx["samples"][rc.list_regexes("cn")[0]]
    text = "cn(geosite:cn)\nrest(all)"
    hosts = [roots[0], "www." + roots[199], "x" + roots[7], roots[100].upper() + ".", sample, "x" + sample + "x",
             "xn--" + roots[0], ""]
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(text), {"cn": 3, "rest": 4}, Geo(), device_regex=True,
                                    device_index=True) as rs, \
            hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(text), {"cn": 3, "rest": 4}, Geo(),
                                       device_regex=True) as lin:
        assert rs.flags() == acl.FLAG_REGEX | acl.FLAG_INDEX and lin.flags() == acl.FLAG_REGEX
        got = rs.match_many([(h, None, None) for h in hosts], [1] * len(hosts), [443] * len(hosts))
        assert got == lin.match_many([(h, None, None) for h in hosts], [1] * len(hosts), [443] * len(hosts))
        assert got == [rs.decision(rs.match_host(h)) for h in hosts]
        assert [g[0] for g in got[:2]] == [3, 3] and got[3][0] == 3 and got[4][0] == 3
        h = rs.device_set(0)
        assert acl.ruleset_index_info(h, 0)[:2] == (200, 512) and acl.ruleset_entries(h) == 1 + 37 + 1
        assert acl.ruleset_entries(lin.device_set(0)) == 200 + 37 + 1
